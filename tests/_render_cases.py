"""Shared by tests/test_render.py (CPU: render_kernel and its host routing on the simulator) and tests/test_render_gpu.py (the real kernel, ops.draw_detections and
YOLOv5.render): the yardstick of the annotated images (include/yolort_amd.h ymi_render), the case tables and ONE driver for both libraries -- the simulator takes host
pointers, libyolort_amd.so device pointers, the call is the same.

The yardstick is a NumPy restatement of the drawing rule of the header, written independently of the kernel: a painter that walks the detections from the LAST slot to
the first and paints outline, label background and text of each with boolean masks (the reference's draw order, yolort/v5/models/common.py:608 `reversed(pred)` with
Annotator.box_label's three calls, yolort/v5/utils/plots.py:98-159), Python's own f"{x:.2f}" for the score text, and a blit of whole character cells from the committed
glyph table (yolort_amd/csrc/render_font.hpp).  Everything is compared bit for bit on images of random bytes; every image is a view inside a larger poisoned buffer,
so "no other pixel and no guard byte changed" is part of every comparison.  PIL.ImageDraw.rectangle is a second yardstick for outlines and backgrounds where the rule
claims to equal it (2 * lw <= min(X1 - X0, Y1 - Y0) + 1); the text has no parity with the reference (it needs a downloaded Arial.ttf or cv2)."""
import ctypes as C
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTS = ("u8hwc", "u8", "f32", "f16", "bf16")
TORCH_DT = {"u8hwc": torch.uint8, "u8": torch.uint8, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DT_CODE = {"f16": 0, "bf16": 1, "f32": 2, "u8": 3, "u8hwc": 4}
BAD_COUNT, STALE_ROW, BAD_LABEL = 1, 2, 4
NAME_STRIDE, MAX_K = 28, 1024
GUARD = 64                                       # guard elements on either side of an image
POISON = {"u8hwc": 0xA5, "u8": 0xA5, "f32": -7.0, "f16": -7.0, "bf16": -7.0}
OUTLINE, BACKGROUND, GLYPH = 1, 2, 3             # what decided a pixel
PALETTE = np.array([[250, 10, 20], [30, 240, 50], [40, 60, 230], [200, 200, 0], [0, 180, 190], [170, 0, 160], [90, 90, 90]], np.uint8)
TXT = (255, 254, 253)
NAN, INF = float("nan"), float("inf")


# ---- the glyph table -------------------------------------------------------------------------------------------------------------------------------------------------
def font_table():
    """(95, 11, 6) bool from the committed file the kernel includes: bit (5 - column) of a row byte"""
    text = open(os.path.join(ROOT, "yolort_amd", "csrc", "render_font.hpp")).read()
    rows = np.array([int(v, 16) for v in re.findall(r"0x([0-9a-f]{2}),", text)], np.uint8)
    assert rows.size == 95 * 11, rows.size
    return ((rows.reshape(95, 11, 1) >> (5 - np.arange(6))) & 1).astype(bool)


FONT = font_table()


def text_bitmap(text, fs):
    """whole cells side by side, every pixel replicated fs x fs -> (11 fs, 6 fs len(text)) bool"""
    cells = [FONT[(ord(ch) if 32 <= ord(ch) <= 126 else ord("?")) - 32] for ch in text]
    return np.kron(np.concatenate(cells, 1), np.ones((fs, fs), bool))


# ---- the rule, in NumPy ----------------------------------------------------------------------------------------------------------------------------------------------
def corners(box):
    """(X0, Y0, X1, Y1) or None when the detection draws nothing"""
    b = [float(v) for v in box]
    if not all(np.isfinite(v) and abs(v) < 2.0 ** 24 for v in b):
        return None
    x0, y0, x1, y1 = (int(v) for v in b)         # int() truncates toward zero
    return None if x1 < x0 or y1 < y0 else (x0, y0, x1, y1)


def label_text(label, score, names, conf):
    """the label's characters: the class name (or its index), then ' ' and the score"""
    name = str(label) if names is None else "".join(chr(c) if 32 <= c <= 126 else "?" for c in names[label][:NAME_STRIDE - 1])
    if not conf:
        return name
    s = np.float32(score)
    return name + " " + (f"{float(s):.2f}" if 0 <= s <= 1 else "?.??")   # Python's own formatting of the fp32 value; NaN fails both comparisons


def masks(h, w, c, lw, fs, text):
    """one detection on an h x w image -> (window, outline, label background, glyph bits): boolean masks over the window (row slice, column slice) that holds all three
    (masks over the whole image say the same and cost a hundred times as much for a slab of small boxes)"""
    x0, y0, x1, y1 = c
    tw, th = 6 * fs * len(text), 11 * fs
    ty = y0 - th if y0 - th >= 0 else y0
    top, left = max(min(y0, ty), 0), max(x0, 0)
    bottom, right = min(max(y1, ty + th + 1 if text else y1) + 1, h), min(max(x1, x0 + tw + 1 if text else x1) + 1, w)
    win = (slice(top, max(bottom, top)), slice(left, max(right, left)))
    ys, xs = np.arange(h)[win[0], None], np.arange(w)[None, win[1]]
    inside = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
    outline = inside & ((xs < x0 + lw) | (xs > x1 - lw) | (ys < y0 + lw) | (ys > y1 - lw))
    back, glyph = np.zeros(outline.shape, bool), np.zeros(outline.shape, bool)
    if text:
        back = (xs >= x0) & (xs <= x0 + tw + 1) & (ys >= ty) & (ys <= ty + th + 1)
        bm = text_bitmap(text, fs)
        ya, yb, xa, xb = max(ty, 0), min(ty + th, h), max(x0, 0), min(x0 + tw, w)
        if ya < yb and xa < xb:
            glyph[ya - top: yb - top, xa - left: xb - left] = bm[ya - ty: yb - ty, xa - x0: xb - x0]
    return win, outline, back, glyph


def paint(img, dets, lw, fs, names, colors, txt, draw_labels, draw_conf, num_classes):
    """img (h, w, 3) uint8, dets [(box, score, label)] in slot order -> (the painted copy, (h, w) map of what decided each pixel (0: untouched), bad-label flag)"""
    out, kind = img.copy(), np.zeros(img.shape[:2], np.uint8)
    bad = False
    h, w = img.shape[:2]
    for box, score, label in reversed(dets):     # the reference paints the last detection first: the first one ends on top
        if not 0 <= label < num_classes:
            bad = True
            continue
        c = corners(box)
        if c is None:
            continue
        text = label_text(label, score, names, draw_conf) if draw_labels else ""
        win, outline, back, glyph = masks(h, w, c, lw, fs, text)
        colour = colors[label % len(colors)]
        o, kd = out[win], kind[win]              # views: painting them paints the image
        o[outline], kd[outline] = colour, OUTLINE
        o[back], kd[back] = colour, BACKGROUND
        o[glyph], kd[glyph] = txt, GLYPH
    return out, kind, bad


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------------------------
def name_table(names):
    t = np.zeros((len(names), NAME_STRIDE), np.uint8)
    for i, nm in enumerate(names):
        t[i, 0] = len(nm)
        t[i, 1: 1 + len(nm)] = list(nm)
    return t


class Case:
    """sizes [(h, w)]; dets: per image the list [(box, score, label)] of ALL k-or-fewer slots handed in; counts: per image as handed in (default: len(dets[i])).  Slots
    at or past a count are poisoned (NaN and huge boxes, NaN scores, labels far outside); names: list of bytes objects or None; claims: the kinds of primitive the
    case is about -- `expected` asserts each of them decided at least one pixel that differs from the input"""

    def __init__(self, name, dt, sizes, dets, lw=2, fs=1, counts=None, k=None, names=None, colors=PALETTE, txt=TXT, draw_labels=True, draw_conf=True, num_classes=None,
                 claims=(OUTLINE,), offset=0, seed=0):
        self.name, self.dt, self.sizes, self.dets = name, dt, list(sizes), [list(d) for d in dets]
        n = len(self.sizes)
        self.lw = [lw] * n if isinstance(lw, int) else list(lw)
        self.fs = [fs] * n if isinstance(fs, int) else list(fs)
        self.counts = [len(d) for d in self.dets] if counts is None else list(counts)
        self.k = max([len(d) for d in self.dets] + [1]) if k is None else k
        self.names, self.colors, self.txt, self.draw_labels, self.draw_conf = names, np.asarray(colors, np.uint8), tuple(txt), draw_labels, draw_conf
        self.num_classes = num_classes if num_classes is not None else (len(names) if names is not None else 1000)
        self.claims, self.offset = tuple(claims), offset
        g = np.random.default_rng(seed + 17 * n + self.k)
        self.inputs = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in self.sizes]
        self.boxes = np.empty((n, self.k, 4), np.float32)
        self.boxes[:, :, :2], self.boxes[:, :, 2:] = NAN, 3.0e9
        self.scores = np.full((n, self.k), NAN, np.float32)
        self.labels = np.full((n, self.k), -(1 << 40), np.int64)
        for i, d in enumerate(self.dets):
            for j, (box, score, label) in enumerate(d):
                self.boxes[i, j], self.scores[i, j], self.labels[i, j] = box, score, label
        self._expected = None

    def expected(self):
        """([painted (h, w, 3) uint8], status), computed once"""
        if self._expected is None:
            outs, status, seen = [], 0, set()
            for i, img in enumerate(self.inputs):
                c = self.counts[i]
                if c < 0:
                    status |= STALE_ROW
                    outs.append(img.copy())
                    continue
                if c > self.k:
                    status |= BAD_COUNT
                live = [(self.boxes[i, j], self.scores[i, j], int(self.labels[i, j])) for j in range(min(c, self.k))]
                out, kind, bad = paint(img, live, self.lw[i], self.fs[i], self.names, self.colors, self.txt, self.draw_labels, self.draw_conf, self.num_classes)
                status |= BAD_LABEL if bad else 0
                changed = (out != img).any(-1)
                seen |= {kd for kd in (OUTLINE, BACKGROUND, GLYPH) if (changed & (kind == kd)).any()}
                outs.append(out)
            assert set(self.claims) <= seen, f"{self.name}: claims {self.claims}, but only {sorted(seen)} decided a pixel that differs from the input"
            self._expected = (outs, status)
        return self._expected


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------------------------------
_LUT = {}


def store(img, dt):
    """(h, w, 3) uint8 -> the flat storage form of the image: interleaved bytes, planar bytes, or planar byte / 255 rounded ONCE to the dtype"""
    t = torch.from_numpy(np.ascontiguousarray(img if dt == "u8hwc" else img.transpose(2, 0, 1))).reshape(-1)
    if dt in ("u8hwc", "u8"):
        return t
    if dt not in _LUT:
        _LUT[dt] = (torch.arange(256, dtype=torch.float64) / 255).to(TORCH_DT[dt])   # float64 -> dtype: one rounding of a quotient that is exact to 2^-53
    return _LUT[dt][t.long()]


def error_text(lib):
    err = getattr(lib, "sim_last_error", None) or lib.ymi_last_error
    err.restype = C.c_char_p
    return err().decode()


def describe(case, ptrs, dev_tensors, keep):
    from yolort_amd._lib import RenderDesc
    n = len(case.sizes)
    d = RenderDesc()
    arr = lambda vals, ty=C.c_int32: (ty * max(len(vals), 1))(*vals)
    p, hw, lw, fs = arr(ptrs, C.c_void_p), arr([v for s in case.sizes for v in s]), arr(case.lw), arr(case.fs)
    keep += [p, hw, lw, fs]
    d.imgs, d.hw, d.lw, d.fs = C.cast(p, C.POINTER(C.c_void_p)), C.cast(hw, C.POINTER(C.c_int32)), C.cast(lw, C.POINTER(C.c_int32)), C.cast(fs, C.POINTER(C.c_int32))
    d.boxes, d.scores, d.labels, d.counts, d.colors, d.status = (dev_tensors[f].data_ptr() for f in ("boxes", "scores", "labels", "counts", "colors", "status"))
    d.status += 4                                # the word between two poisoned ones
    d.names = dev_tensors["names"].data_ptr() if case.names is not None else None
    d.m, d.num_classes, d.in_dtype = len(case.colors), case.num_classes, DT_CODE[case.dt]
    for i in range(3):
        d.txt_color[i] = case.txt[i]
    d.draw_labels, d.draw_conf, d.n, d.k = int(case.draw_labels), int(case.draw_conf), n, case.k
    return d


def buffers(case, device):
    """every image inside its own poisoned buffer [GUARD | offset | image | GUARD], the slab and the tables -> (image buffers, tensors)"""
    bufs = []
    for img in case.inputs:
        flat = store(img, case.dt)
        buf = torch.full((GUARD + case.offset + flat.numel() + GUARD,), POISON[case.dt], dtype=TORCH_DT[case.dt])
        buf[GUARD + case.offset: GUARD + case.offset + flat.numel()] = flat
        bufs.append(buf.to(device))
    t = dict(boxes=torch.from_numpy(case.boxes), scores=torch.from_numpy(case.scores), labels=torch.from_numpy(case.labels), counts=torch.tensor(case.counts, dtype=torch.int32),
             colors=torch.from_numpy(case.colors), status=torch.tensor([-77, 0, -77], dtype=torch.int32),
             names=torch.from_numpy(name_table(case.names if case.names is not None else [b""])))
    return bufs, {f: v.to(device) for f, v in t.items()}


def run_render(lib, case, device="cpu", stream=None):
    """ymi_render of `case` -> (image buffers on the host after the call, the three status words)"""
    lib.ymi_render.restype = C.c_int
    bufs, t = buffers(case, device)
    keep = []
    d = describe(case, [b.data_ptr() + (GUARD + case.offset) * b.element_size() for b in bufs], t, keep)
    rc = lib.ymi_render(C.byref(d), stream)
    assert rc == 0, (case.name, rc, error_text(lib))
    if device != "cpu":
        torch.cuda.synchronize()
    return [b.cpu() for b in bufs], t["status"].cpu().tolist()


def check(result, case):
    """bit for bit: every image equals the painter's, every guard element and the words around the status are untouched, the status word is the expected one"""
    bufs, status = result
    want, want_status = case.expected()
    assert status == [-77, want_status, -77], (case.name, status, want_status)
    for i, buf in enumerate(bufs):
        flat = store(want[i], case.dt)
        a = GUARD + case.offset
        got = buf[a: a + flat.numel()]
        if not torch.equal(got, flat):
            h, w = case.sizes[i]
            diff = (got != flat).reshape((h, w, 3) if case.dt == "u8hwc" else (3, h, w))
            where = torch.nonzero(diff)[:5].tolist()
            raise AssertionError(f"{case.name}: image {i} ({h} x {w}) differs in {int(diff.sum())} elements, first at {where}")
        assert (buf[:a] == POISON[case.dt]).all() and (buf[a + flat.numel():] == POISON[case.dt]).all(), f"{case.name}: a guard element of image {i} was written"
    return want


# ---- the case tables -------------------------------------------------------------------------------------------------------------------------------------------------
def det(x0, y0, x1, y1, score=0.5, label=0):
    return ((x0, y0, x1, y1), score, label)


def sweep_boxes(g, h, w, count):
    """boxes of a few pixels around and across an h x w image, with the odd ones out: degenerate (a point, a line), inverted, wholly outside, non-finite, 2^30"""
    out = []
    for j in range(count):
        x0, y0 = g.uniform(-10, w + 4), g.uniform(-10, h + 4)
        box = [x0, y0, x0 + g.uniform(0, w * 0.8 + 6), y0 + g.uniform(0, h * 0.8 + 6)]
        odd = g.integers(0, 12)
        if odd == 0:
            box[2], box[3] = box[0], box[1]                      # a point
        elif odd == 1:
            box[2] = box[0] - g.uniform(1, 5)                    # inverted
        elif odd == 2:
            box = [w + 3.5, 1.0, w + 9.0, h - 1.0]               # wholly outside
        elif odd == 3:
            box[int(g.integers(0, 4))] = [NAN, INF, -INF, 2.0 ** 30, -2.0 ** 30, 2.0 ** 24][int(g.integers(0, 6))]
        elif odd == 4:
            box = [-3.0, -3.0, w + 3.0, h + 3.0]                 # around the whole image
        out.append((tuple(box), float(g.uniform(0, 1)), int(g.integers(0, 40))))
    return out


def geometry_sweep(dt, seed=0):
    """66 images (two launches) with sides 1..40, lw 1..7, six boxes each, labels = the class index with its score"""
    g = np.random.default_rng(100 + seed)
    sizes = [(int(g.integers(1, 41)), int(g.integers(1, 41))) for _ in range(66)]
    sizes[0], sizes[64], sizes[65] = (1, 1), (40, 40), (17, 1)
    dets = [sweep_boxes(g, h, w, 6) for h, w in sizes]
    dets[64][0] = det(3.7, 14.2, 30.9, 35.5, 0.25, 7)            # the images of the second launch are certainly drawn on
    dets[65][0] = det(-2.0, 2.0, 5.0, 9.0, 0.25, 7)
    return Case(f"sweep-{dt}", dt, sizes, dets, lw=[1 + i % 7 for i in range(66)], claims=(OUTLINE, BACKGROUND, GLYPH), seed=seed)


PIL_BATCHES, PIL_MIN_PER_BATCH = 8, 25           # 8 x 64 cases, of which those with 2 * lw <= min side + 1 take part: at least 25 a batch, 200 in all


def pil_batch(b):
    """64 interleaved images with ONE box each and a label of one blank (conf off): outline and background and no set glyph bit, so the whole image is PIL's"""
    g = np.random.default_rng(500 + b)
    sizes, dets, lws = [], [], []
    for _ in range(64):
        h, w = int(g.integers(8, 40)), int(g.integers(8, 40))
        x0, y0 = float(g.uniform(-10, w - 4)), float(g.uniform(-10, h - 4))
        bw, bh = float(g.uniform(2, w)), float(g.uniform(2, h))
        sizes.append((h, w))
        lws.append(int(g.integers(1, 8)))
        dets.append([det(x0, y0, x0 + bw, y0 + bh, 0.5, int(g.integers(0, 7)))])
    return Case(f"pil-{b}", "u8hwc", sizes, dets, lw=lws, names=[b" "] * 7, draw_conf=False, claims=(OUTLINE, BACKGROUND), seed=b)


def pil_takes_part(case, i):
    c = corners(case.dets[i][0][0])
    return c is not None and 2 * case.lw[i] <= min(c[2] - c[0], c[3] - c[1]) + 1


def pil_image(case, i):
    """the same drawing with PIL.ImageDraw.rectangle: outline of width lw, then the filled label background"""
    from PIL import Image, ImageDraw
    (box, _, label), fs = case.dets[i][0], case.fs[i]
    x0, y0, x1, y1 = corners(box)
    colour = tuple(int(v) for v in case.colors[label % len(case.colors)])
    im = Image.fromarray(case.inputs[i].copy())
    draw = ImageDraw.Draw(im)
    draw.rectangle([x0, y0, x1, y1], width=case.lw[i], outline=colour)
    tw, th = 6 * fs * 1, 11 * fs
    ty = y0 - th if y0 - th >= 0 else y0
    draw.rectangle([x0, ty, x0 + tw + 1, ty + th + 1], fill=colour)
    return np.asarray(im)


def tiles_case(dt, offset=0):
    """the tile is 64 x 16: box edges on x = 63 / 64 and y = 15 / 16, outlines straddling tile boundaries, widths 1, 65 and 37 (odd), a width that is a multiple of 4
    (the vector stores; with offset = 1 the view is misaligned and takes the scalar ones), an image smaller than a tile"""
    sizes = [(40, 132), (20, 1), (20, 65), (33, 37), (5, 7), (34, 68)]
    dets = [[det(10, 3, 63, 15, 0.5, 0), det(64, 16, 100, 31, 0.5, 1), det(50, 10, 80, 20, 0.5, 2), det(62, 14, 66, 18, 0.5, 3), det(100, 0, 131, 39, 0.5, 4), det(0, 32, 127, 32, 0.5, 5)],
            [det(0, 2, 0, 9, 0.5, 0), det(-3, 12, 5, 18, 0.5, 1)],
            [det(60, 1, 64, 18, 0.5, 2), det(0, 15, 64, 16, 0.5, 3)],
            [det(1, 1, 35, 31, 0.5, 4), det(30, 14, 40, 18, 0.5, 5)],
            [det(1, 1, 5, 3, 0.5, 6), det(-5, -5, 20, 20, 0.5, 0)],
            [det(4, 4, 63, 29, 0.5, 1), det(0, 0, 67, 33, 0.5, 2), det(8, 8, 11, 8, 0.5, 3)]]
    return Case(f"tiles-{dt}-off{offset}", dt, sizes, dets, lw=3, draw_labels=False, offset=offset)


def one_tile_case(dt="u8hwc"):
    """three images of 3 x 3 tiles each; ONE tile of the middle image is touched"""
    return Case(f"one-tile-{dt}", dt, [(48, 192)] * 3, [[], [det(70, 18, 120, 29, 0.5, 1)], []], lw=2, draw_labels=False, k=4)


def order_case(dt="u8hwc"):
    """three overlapping boxes of distinct colours; a low-priority label background under a high-priority outline and the reverse"""
    names = [b"ab", b"cd", b"ef", b"gh"]
    dets = [[det(5, 20, 40, 45, 0.5, 0), det(20, 30, 60, 55, 0.6, 1), det(10, 25, 50, 50, 0.7, 2)],
            [det(10, 14, 60, 40, 0.5, 0), det(8, 30, 70, 50, 0.5, 1)],      # slot 1's label (rows 19..31) lies under slot 0's outline
            [det(8, 30, 70, 50, 0.5, 1), det(10, 14, 60, 40, 0.5, 0)]]      # ... and over it
    return Case(f"order-{dt}", dt, [(64, 80)] * 3, dets, lw=3, names=names, claims=(OUTLINE, BACKGROUND, GLYPH))


def full_slab_case(dt="u8hwc"):
    """k = 1024 boxes that all cover the one 16 x 64 tile of the image"""
    g = np.random.default_rng(9)
    dets = [det(float(g.uniform(-5, 30)), float(g.uniform(-5, 7)), float(g.uniform(31, 70)), float(g.uniform(8, 20)), 0.5, int(g.integers(0, 7))) for _ in range(MAX_K)]
    return Case(f"full-slab-{dt}", dt, [(16, 64)], [dets], lw=1, draw_labels=False, k=MAX_K)


def label_case(fs, dt="u8hwc", **kw):
    """labels at scale fs: Y0 - h == 0 (outside, the label starts in row 0), Y0 - h == -1 (inside), labels running off the right and the bottom edge, an empty name, a
    27-byte name, a byte outside 32..126"""
    th = 11 * fs
    names = [b"cat", b"", b"abcdefghijklmnopqrstuvwxyz~", b"d\x07g\xe9", b"{|}"]
    hh, ww = 4 * th + 30, 6 * fs * 12 + 20
    dets = [[det(3, th, 40, th + 9, 0.87, 0), det(3, 3 * th, 30, 3 * th + 8, 0.05, 4)],                       # outside, starting in row 0
            [det(3, th - 1, 40, th + 9, 0.87, 0)],                                                           # one row short: inside
            [det(ww - 20, 2 * th, ww + 5, 2 * th + 12, 1.0, 0), det(2, hh - 6, 20, hh + 3, 0.0, 3)],          # off the right edge; a box across the bottom edge
            [det(2, 2 * th, 30, 2 * th + 9, 0.33, 1), det(2, 4 * th, 30, 4 * th + 6, 0.5, 2), det(40, 2 * th, 60, 2 * th + 9, 0.99, 3)],
            [det(2, 5, 30, th + 20, 0.5, 0)]]                                                                # an image of th + 8 rows: the label is inside and runs off the bottom edge
    claims = (OUTLINE, BACKGROUND, GLYPH) if kw.get("draw_labels", True) else (OUTLINE,)
    return Case(f"labels-fs{fs}-{dt}" + "".join(f"-{k}" for k in kw), dt, [(hh, ww)] * 4 + [(th + 8, ww)], dets, lw=2, fs=fs, names=names, claims=claims, **kw)


def index_label_case(dt="u8hwc"):
    """names = null: the class index in decimal, one to ten digits"""
    dets = [[det(2, 12 + 24 * j, 90, 20 + 24 * j, 0.5, lab) for j, lab in enumerate((0, 7, 10, 409, 65535, 2147483646))]]
    return Case(f"index-labels-{dt}", dt, [(160, 110)], dets, lw=1, names=None, num_classes=2147483647, claims=(OUTLINE, BACKGROUND, GLYPH))


def score_values():
    """at least 512 fp32 scores: the exact ties, the fp32 neighbours of 0.005 and 0.995 on both sides, 0, -0, 1, the "?.??" class, hundredths-and-a-half, random ones"""
    f = np.float32
    v = [f(0.125), f(0.375), f(0.625), f(0.875), f(0.0), f(-0.0), f(1.0), f(NAN), f(1.5), f(-0.1), f(INF), f(-INF), f(1.0000001), f(-1e-45)]
    for c in (0.005, 0.995):
        v += [f(c), np.nextafter(f(c), f(-1)), np.nextafter(f(c), f(2))]
    v += [f((2 * i + 1) / 200) for i in range(100)]
    v += list(np.random.default_rng(3).uniform(0, 1, 520 - len(v)).astype(f))
    return np.array(v, f)


def scores_case(dt="u8hwc"):
    """the scores drawn as stacks of small boxes, 40 to a column, each with the label " d.dd" (an empty name) above it"""
    vals = score_values()
    dets = [det(2 + 42 * (j // 40), 11 + 14 * (j % 40), 36 + 42 * (j // 40), 12 + 14 * (j % 40), float(s), 0) for j, s in enumerate(vals)]
    for j, s in enumerate(vals):
        dets[j] = (dets[j][0], s, 0)             # the fp32 value itself (NaN and -0.0 included)
    return Case(f"scores-{dt}", dt, [(14 * 40 + 4, 42 * 13 + 4)], [dets], lw=1, names=[b""], claims=(OUTLINE, BACKGROUND, GLYPH))


def counts_case(counts, dt="u8hwc", bad_label=False):
    """four images, k = 4, three live detections handed in per image and whatever `counts` says; slots at or past a count hold the poison of Case"""
    dets = [[det(2 + 3 * j, 13 + 2 * j, 40 + 3 * j, 30 + 2 * j, 0.5, j) for j in range(4)] for _ in range(4)]
    if bad_label:
        dets[1][1] = (dets[1][1][0], 0.5, 7)     # == num_classes
        dets[2][0] = (dets[2][0][0], 0.5, -1)
    return Case(f"counts-{counts}-{dt}-{bad_label}", dt, [(40, 70)] * 4, dets, counts=counts, k=4, names=[b"a", b"b", b"c", b"d", b"e", b"f", b"g"], claims=(OUTLINE, BACKGROUND, GLYPH))


def refusals():
    """(what, change(d) applied to a valid descriptor, a word of the message) for every refusal of ymi_render"""
    def setter(**kw):
        def f(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return f

    def host(field, value):
        def f(d):
            arr = (C.c_int32 * 8)(*([2] * 8))
            arr[1] = value
            setattr(d, field, C.cast(arr, C.POINTER(C.c_int32)))
            d._keep = arr
        return f

    def txt(d):
        d.txt_color[1] = 256

    out = [(f"null {f}", setter(**{f: None}), "null") for f in ("imgs", "hw", "lw", "fs", "boxes", "scores", "labels", "counts", "colors", "status")]
    out += [("k 1025", setter(k=MAX_K + 1), "YMI_RENDER_MAX_K"), ("n -1", setter(n=-1), "negative"), ("k -1", setter(k=-1), "negative"), ("lw 0", host("lw", 0), "lw[1]"),
            ("lw -3", host("lw", -3), "lw[1]"), ("fs 0", host("fs", 0), "fs[1]"), ("m 0", setter(m=0), "colours"), ("in_dtype 5", setter(in_dtype=5), "in_dtype"),
            ("in_dtype -1", setter(in_dtype=-1), "in_dtype"), ("num_classes 0", setter(num_classes=0), "classes"), ("txt 256", txt, "txt_color")]
    return out


def check_refusals(lib, device="cpu"):
    """every refusal returns YMI_EINVAL with a message and writes nothing; n == 0 is accepted with every buffer null"""
    from yolort_amd._lib import RenderDesc
    case = counts_case([3, 3, 3, 3])
    bufs, t = buffers(case, device)
    before = [b.cpu().clone() for b in bufs]
    ptrs = [b.data_ptr() + (GUARD + case.offset) * b.element_size() for b in bufs]
    lib.ymi_render.restype = C.c_int
    assert lib.ymi_render(None, None) == -1
    for what, change, word in refusals():
        keep = []
        d = describe(case, ptrs, t, keep)
        change(d)
        rc = lib.ymi_render(C.byref(d), None)
        assert rc == -1 and word in error_text(lib), (what, rc, error_text(lib))
    keep = []
    d = describe(case, ptrs, t, keep)
    null_image = (C.c_void_p * len(ptrs))(*ptrs)
    null_image[2] = None
    d.imgs = C.cast(null_image, C.POINTER(C.c_void_p))
    assert lib.ymi_render(C.byref(d), None) == -1 and "image 2" in error_text(lib)
    empty = RenderDesc()
    assert lib.ymi_render(C.byref(empty), None) == 0, "n == 0 with every buffer null is an empty batch"
    if device != "cpu":
        torch.cuda.synchronize()
    assert all(torch.equal(b.cpu(), a) for b, a in zip(bufs, before)) and t["status"].cpu().tolist() == [-77, 0, -77], "a refused call wrote something"
