"""Shared by tests/test_nv12_draw.py (CPU: the RGB -> YCbCr contract, render_nv12_kernel on the simulator) and tests/test_nv12_draw_gpu.py (the real kernels): NumPy
restatements of the contract (include/yolort_amd.h, "NV12 drawing and cropping"), the expected planes built from tests/_render_cases.py's painter, the case table and
ONE driver of ymi_render_nv12 -- the simulator takes host pointers, libyolort_amd.so device pointers.  Everything is compared bit for bit on planes of random bytes
that sit, with their pitch padding, inside poisoned buffers: "no other byte changed" is part of every comparison."""
import ctypes as C
import functools
from typing import NamedTuple, Tuple

import numpy as np
import torch

import _render_cases as T
from _nv12_cases import K
from _render_cases import BAD_COUNT, BAD_LABEL, STALE_ROW, Case, det, paint
from yolort_amd import _lib

YCC_BOUND = 0.5 + 3 * 255 * 2.0 ** -15           # the rounding shift + three coefficients each off by at most 2^-15, times values <= 255
COLORS = np.random.default_rng(5).integers(0, 256, (7, 3), dtype=np.uint8)   # a seeded random palette: the conversion runs on the device
TXT = (251, 3, 130)                              # not a palette colour
GUARD, POISON = 64, 0xA5


def ycc_int(rgb, matrix, full, clamp=True):
    """the integer rule in int64: (..., 3) RGB -> (..., 3) uint8 {Y, Cb, Cr}; clamp=False: the int64 codes before the clamp"""
    c = np.array(_lib.YCC_COEF[(matrix, full)], np.int64).reshape(3, 3)
    v = ((rgb.astype(np.int64) @ c.T + 8192) >> 14) + np.array([0 if full else 16, 128, 128])
    return np.clip(v, 0, 255).astype(np.uint8) if clamp else v


def ycc_real(rgb, matrix, full):
    """the real-valued formula in float64, not clamped and not rounded"""
    kr, kb = K[matrix]
    r, g, b = (rgb[..., i].astype(np.float64) for i in range(3))
    y = kr * r + (1 - kr - kb) * g + kb * b
    cb, cr = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    return np.stack([y, cb + 128, cr + 128] if full else [y * 219 / 255 + 16, cb * 224 / 255 + 128, cr * 224 / 255 + 128], -1)


class NvDraw(NamedTuple):
    case: Case                                   # the slab, the tables and the flags (its images are not used)
    frames: Tuple[Tuple[int, ...], ...]          # per frame (h, w, pitch_y, pitch_uv, Y base offset, CbCr base offset)
    matrix: str = "bt601"
    full: bool = False


def fr(h, w, py=None, puv=None, oy=0, ouv=0):
    return (h, w, py or w, puv or w, oy, ouv)


def make(name, frames, dets, matrix="bt601", full=False, **kw):
    return NvDraw(Case(name, "u8hwc", [f[:2] for f in frames], dets, colors=COLORS, txt=TXT, **kw), tuple(frames), matrix, full)


@functools.lru_cache(maxsize=None)
def planes(nd):
    """random planes with their pitch: [(y (h, pitch_y), uv (h / 2, pitch_uv))]"""
    g = np.random.default_rng(len(nd.frames) + nd.case.k)
    return [(g.integers(0, 256, (f[0], f[2]), dtype=np.uint8), g.integers(0, 256, (f[0] // 2, f[3]), dtype=np.uint8)) for f in nd.frames]


@functools.lru_cache(maxsize=None)
def expected(nd):
    """-> ([(Y plane, CbCr plane)] with their padding, status, the set of raster positions that were "first decided", whether a 2 x 2 block carries two colours)"""
    c, outs, status, firsts, mixed = nd.case, [], 0, set(), False
    for i, ((y, uv), (h, w, *_)) in enumerate(zip(planes(nd), nd.frames)):
        y, uv, cnt = y.copy(), uv.copy(), c.counts[i]
        status |= STALE_ROW if cnt < 0 else (BAD_COUNT if cnt > c.k else 0)
        live = [(c.boxes[i, j], c.scores[i, j], int(c.labels[i, j])) for j in range(max(min(cnt, c.k), 0))]
        rgb, kind, bad = paint(np.zeros((h, w, 3), np.uint8), live, c.lw[i], c.fs[i], c.names, c.colors, c.txt, c.draw_labels, c.draw_conf, c.num_classes)
        status |= BAD_LABEL if bad else 0
        ycc, dec = ycc_int(rgb, nd.matrix, nd.full), kind != 0
        y[:, :w][dec] = ycc[..., 0][dec]
        blocks = lambda a: a.reshape(h // 2, 2, w // 2, 2, -1).swapaxes(1, 2).reshape(h // 2, w // 2, 4, -1)   # noqa: E731  the 2 x 2 blocks in raster order
        d4, c4 = blocks(dec)[..., 0], blocks(ycc[..., 1:])
        first, hit = d4.argmax(-1), d4.any(-1)
        pairs = uv[:, :w].reshape(h // 2, w // 2, 2)
        pairs[hit] = np.take_along_axis(c4, first[..., None, None], 2)[:, :, 0][hit]
        uv[:, :w] = pairs.reshape(h // 2, w)
        firsts |= set(first[hit].tolist())
        mixed |= bool(((c4 != c4[:, :, :1]).any(-1) & d4 & d4[:, :, :1]).any())
        outs.append((y, uv))
    return outs, status, firsts, mixed


def _buffer(arr, off, device):
    buf = torch.full((GUARD + off + arr.size + GUARD,), POISON, dtype=torch.uint8)
    buf[GUARD + off: GUARD + off + arr.size] = torch.from_numpy(arr).reshape(-1)
    return buf.to(device)


def describe(nd, device="cpu", change=None):
    """-> (descriptor, plane buffers [y0, uv0, y1, ...] on the device, status tensor, everything that must stay alive); change(d, keep) edits the valid descriptor"""
    c, n = nd.case, len(nd.frames)
    bufs = [_buffer(p, f[4 + j], device) for pl, f in zip(planes(nd), nd.frames) for j, p in enumerate(pl)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    ptr = lambda i, j: bufs[2 * i + j].data_ptr() + GUARD + nd.frames[i][4 + j]   # noqa: E731
    _, t = T.buffers(Case("slab", "u8hwc", [(1, 1)], [[]], names=c.names, colors=c.colors), device)
    t.update({f: torch.from_numpy(getattr(c, f)).to(device) for f in ("boxes", "scores", "labels")}, counts=torch.tensor(c.counts, dtype=torch.int32).to(device))
    arr = lambda vals, ty=C.c_int32: (ty * len(vals))(*vals)   # noqa: E731
    keep = [arr([ptr(i, 0) for i in range(n)], C.c_void_p), arr([ptr(i, 1) for i in range(n)], C.c_void_p), arr([v for f in nd.frames for v in f[2:4]]),
            arr([v for f in nd.frames for v in f[:2]]), arr(c.lw), arr(c.fs), t]
    d = _lib.RenderNv12Desc()
    d.y, d.uv = C.cast(keep[0], C.POINTER(C.c_void_p)), C.cast(keep[1], C.POINTER(C.c_void_p))
    d.pitch, d.hw, d.lw, d.fs = (C.cast(a, C.POINTER(C.c_int32)) for a in keep[2:6])
    d.boxes, d.scores, d.labels, d.counts, d.colors = (t[f].data_ptr() for f in ("boxes", "scores", "labels", "counts", "colors"))
    d.status = t["status"].data_ptr() + 4        # the word between two poisoned ones
    d.names = t["names"].data_ptr() if c.names is not None else None
    d.m, d.num_classes, d.matrix, d.range = len(c.colors), c.num_classes, _lib.NV12_MATRIX[nd.matrix], int(nd.full)
    for i in range(3):
        d.txt_color[i] = c.txt[i]
    d.draw_labels, d.draw_conf, d.n, d.k = int(c.draw_labels), int(c.draw_conf), n, c.k
    if change:
        change(d, keep)
    return d, bufs, t["status"], keep


def launch(lib, nd, device="cpu", change=None):
    """one ymi_render_nv12 call -> (rc, plane buffers, status tensor)"""
    d, bufs, status, keep = describe(nd, device, change)
    lib.ymi_render_nv12.restype = C.c_int
    return lib.ymi_render_nv12(C.byref(d), None), bufs, status


def compare(nd, bufs, status, want=None):
    """every buffer -- guard bands, base offset, pitch padding and all -- equals the expected one bit for bit; want = "input": the untouched input"""
    outs, want_status, _, _ = expected(nd)
    outs = planes(nd) if want == "input" else outs
    assert status.cpu().tolist() == [-77, 0 if want == "input" else want_status, -77], (nd.case.name, status.cpu().tolist(), want_status)
    for i, f in enumerate(nd.frames):
        for j, name in enumerate(("Y", "CbCr")):
            got, exp = bufs[2 * i + j].cpu(), _buffer(outs[i][j], f[4 + j], "cpu")
            if not torch.equal(got, exp):
                pos = (torch.nonzero(got != exp)[:5, 0] - GUARD - f[4 + j]).tolist()
                raise AssertionError(f"{nd.case.name}: the {name} buffer of frame {i} ({f}) differs in {int((got != exp).sum())} bytes, first at plane offsets {pos}")


def check(lib, nd, device="cpu"):
    rc, bufs, status = launch(lib, nd, device)
    assert rc == 0, (nd.case.name, T.error_text(lib))
    if device != "cpu":
        torch.cuda.synchronize()
    compare(nd, bufs, status)


# ---- the case table: the smallest shapes at which the kernel can go wrong ------------------------------------------------------------------------------------------
NAMES = [b"ab", b"cat", b"", b"d~"]
_TINY = [fr(2 + 2 * (i % 3), 2 + 2 * (i % 5)) for i in range(66)]
CASES = {c.case.name: c for c in (
    # one pair; a row crossing the 64-column edge; a column crossing the 16-row edge; exactly one tile; both edges
    make("shapes", [fr(2, 2), fr(2, 66), fr(18, 2), fr(16, 64), fr(18, 66)],
         [[det(0, 0, 1, 1)], [det(1, 0, 65, 1, 0.5, 1), det(60, 1, 70, 5, 0.5, 2)], [det(0, 3, 1, 17, 0.5, 3)], [det(3, 2, 62, 13, 0.5, 4), det(0, 0, 63, 15, 0.5, 5)],
          [det(5, 3, 65, 17, 0.5, 6), det(62, 14, 66, 18, 0.5, 0)]], lw=1, draw_labels=False),
    # pitch > width and the Y base at byte offsets 0 / 1 / 2 / 3 with the chroma base at 0 / 2: the dword stores, the byte stores and rows that mix them (odd pitch_y / 2)
    make("pitch-align", [fr(18, 66, 72, 70, oy, ouv) for oy, ouv in ((0, 0), (1, 2), (2, 0), (3, 2))] + [fr(18, 66, 70, 72, 2, 2)],
         [[det(1, 1, 64, 16, 0.5, j), det(20, 5, 40, 12, 0.5, j + 1)] for j in range(5)], lw=6, draw_labels=False),
    # box edges on each parity: every one of the four raster positions is the first decided one of some block
    make("parity", [fr(20, 36)], [[det(3, 3, 12, 11, 0.5, 1), det(16, 4, 31, 14, 0.5, 2)]], lw=1, draw_labels=False),
    # two overlapping boxes of different classes, outlines one pixel apart: blocks carry two colours; labels whose glyph pixels lie inside blocks
    make("overlap", [fr(40, 80)], [[det(5, 14, 50, 35, 0.87, 0), det(7, 15, 60, 38, 0.05, 1), det(30, 2, 70, 30, 1.0, 3)]], lw=2, names=NAMES,
         claims=(T.OUTLINE, T.BACKGROUND, T.GLYPH)),
    # an empty-list tile beside a full one, and a frame with no detection at all
    make("one-tile", [fr(16, 128), fr(4, 4)], [[det(70, 2, 120, 13, 0.5, 1)], []], lw=2, draw_labels=False, k=3),
    # 66 tiny frames: two launches
    make("n66", _TINY, [[det(i % 3 - 1, i % 2, 1 + i % 7, 1 + i % 4, 0.5, i % 7)] for i in range(66)], lw=1, draw_labels=False),
    # status bits: a count above k, a stale row, a label outside the names
    make("status", [fr(12, 20)] * 3, [[det(1, 1, 18, 10, 0.5, 0), det(3, 3, 9, 9, 0.5, 1)], [det(1, 1, 18, 10, 0.5, 0)], [det(2, 2, 15, 9, 0.5, 4), det(4, 0, 19, 11, 0.5, 2)]],
         lw=1, names=NAMES, counts=[3, -1, 2], k=2, draw_labels=False),
)}


def check_claims():
    """the cases exercise what they are about (computed from the expected planes, once)"""
    assert expected(CASES["parity"])[2] == {0, 1, 2, 3} and expected(CASES["overlap"])[3] and expected(CASES["status"])[1] == BAD_COUNT | STALE_ROW | BAD_LABEL
    for nd in CASES.values():
        nd.case.expected()   # the painter's own claims (outline / background / glyph pixels exist)


def check_refusals(lib, device="cpu"):
    """an odd side, an odd pitch, a pitch below the width, an odd chroma pointer, k > 1024, a bad matrix: YMI_EINVAL with a message, nothing launched, nothing written"""
    def host(index, pos, value):
        def f(d, keep):
            keep[index][pos] = value
        return f

    def odd_uv(d, keep):
        keep[1][0] += 1
    nd = CASES["pitch-align"]
    for change in (host(3, 0, 17), host(3, 1, 65), host(3, 0, 0), host(2, 0, 71), host(2, 1, 64), odd_uv, lambda d, keep: setattr(d, "k", T.MAX_K + 1),
                   lambda d, keep: setattr(d, "matrix", 2), lambda d, keep: setattr(d, "range", -1)):
        rc, bufs, status = launch(lib, nd, device, change=change)
        assert rc == -1 and "ymi_render_nv12" in T.error_text(lib), (rc, T.error_text(lib))
        compare(nd, bufs, status, want="input")
