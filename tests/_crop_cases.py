"""Shared by tests/test_crop.py (CPU: crop_resize_kernel and its host routing on the simulator) and tests/test_crop_gpu.py (the real kernel, ops.crop_detections and
YOLOv5.crop): the yardsticks of the detection crops (include/yolort_amd.h ymi_crop_resize), the case tables and ONE driver for both libraries -- the simulator takes
host pointers, libyolort_amd.so device pointers, the call is the same.

Restated from the reference (its yolort.v5 modules are not imported: importing them tries to fetch a font):
  save_one_box   yolort/v5/utils/plots.py:545-558     b = xyxy2xywh(xyxy); square: both sides max(w, h); b[:, 2:] * gain + pad; xywh2xyxy(b).long(); clip_coords
  xyxy2xywh      yolort/v5/utils/general.py:391-401   ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1)
  xywh2xyxy      yolort/v5/utils/general.py:404-414   (x - w / 2, y - h / 2, x + w / 2, y + h / 2)
  clip_coords    yolort/v5/utils/general.py:504-510   x clamped into [0, W], y into [0, H] (on the integers .long() left)
tests/golden/crop_rects.json holds what the reference's own functions give (tests/golden/make_crop_golden.py); `rect_ref` below must reproduce it exactly.
The resize yardstick is F.interpolate(mode="bilinear", align_corners=False) of the cut-out (cv2 is not on the build machine; cv2.resize on uint8 uses fixed-point
weights and differs in the last bit of a byte)."""
import ctypes as C
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import _tta_cases

F32 = np.float32
GUARD = -7.0                                   # poison of the crops' rows and guard bands; the index and total buffers hold int(GUARD)
K = 4                                          # slab depth of every case
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
DT_CODE = {"f16": 0, "bf16": 1, "f32": 2, "u8": 3, "u8hwc": 4}
IN_DTS, OUT_DTS = ("f32", "f16", "bf16", "u8", "u8hwc"), ("f16", "bf16", "f32")
STATUS_CAPACITY, STATUS_BAD_COUNT = 1, 2
SIZES = ((8, 8), (16, 12), (7, 5))             # (out_h, out_w): two widths that take the wide stores, one that takes the scalar form
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crop_rects.json")


# ---- the rectangle -------------------------------------------------------------------------------------------------------------------------------------------------
def rect_ref(boxes, h, w, gain=1.02, pad=10, square=False):
    """save_one_box's rectangle in torch fp32, operation for operation: (m, 4) boxes -> (m, 4) int64 {x1, y1, x2, y2}, empty rectangles with the clipped corners the
    reference leaves them.  One rule of the library on top: a non-finite coordinate (of the box or of a corner) gives (0, 0, 0, 0) -- the reference is undefined there."""
    b = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    g, p, two = torch.tensor(gain, dtype=torch.float32), torch.tensor(pad, dtype=torch.float32), torch.tensor(2.0, dtype=torch.float32)
    cx, cy = (b[:, 0] + b[:, 2]) / two, (b[:, 1] + b[:, 3]) / two
    bw, bh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    if square:
        bw = bh = torch.where(bw > bh, bw, bh)
    bw, bh = bw * g + p, bh * g + p
    c = torch.stack((cx - bw / two, cy - bh / two, cx + bw / two, cy + bh / two), 1)
    finite = torch.isfinite(b).all(1) & torch.isfinite(c).all(1)
    r = torch.where(finite[:, None], c, torch.zeros_like(c)).long()
    r[:, 0::2] = r[:, 0::2].clamp(0, w)
    r[:, 1::2] = r[:, 1::2].clamp(0, h)
    r[~finite] = 0
    return r


def is_empty(rect):
    return int(rect[2]) <= int(rect[0]) or int(rect[3]) <= int(rect[1])


def golden_groups():
    with open(GOLDEN) as f:
        return json.load(f)["groups"]


# ---- the pixels ----------------------------------------------------------------------------------------------------------------------------------------------------
def widen(im, in_dt):
    """the stored image -> (3, h, w) fp32 values as the kernel reads them: uint8 is a true division by 255 (common.hpp load_elem), interleaved images are permuted"""
    if in_dt == "u8hwc":
        return im.permute(2, 0, 1).float() / 255.0
    return im.float() / 255.0 if in_dt == "u8" else im.float()


def crop_ref(im32, rect, size, mean=None, std=None):
    """F.interpolate of the cut-out, fp32; with normalisation the two operations in float64 on torch's fp32 pixels (see pixel_tolerance) -> (3, out_h, out_w) float64"""
    x1, y1, x2, y2 = (int(v) for v in rect)
    if x2 <= x1 or y2 <= y1:
        return torch.zeros((3,) + tuple(size), dtype=torch.float64)
    out = F.interpolate(im32[None, :, y1:y2, x1:x2], size=tuple(size), mode="bilinear", align_corners=False)[0]
    if mean is None:
        return out.double()
    m, s = (torch.tensor(v, dtype=torch.float32).double().view(3, 1, 1) for v in (mean, std))
    return (out.double() - m) / s


def crop_ref_fp32(im32, rect, size, mean, std):
    """the same with the normalisation in torch fp32: what the kernel must equal bit for bit wherever the resize itself is exact"""
    out = crop_ref(im32, rect, size).float()
    if mean is None or is_empty(rect):
        return out
    m, s = (torch.tensor(v, dtype=torch.float32).view(3, 1, 1) for v in (mean, std))
    return (out - m) / s


def pixel_tolerance(out_dt, mean=None, std=None):
    """|kernel - yardstick| for images in [0, 1].
    Resize: the arithmetic of scale_view_kernel on values in [0, 1] -- _tta_cases.scale_tolerance("f32") = 10 * 2^-24 (five roundings of the pixel range on either side).
    Normalisation (v - mean[c]) / std[c]: the yardstick evaluates it in float64 on torch's fp32 pixel, so only the kernel's two fp32 roundings count.  With u = 2^-24:
    a = fl(v - m) has |v - m| <= max(m, 1 - m) <= 1, error <= u; fl(a / s) adds u |a / s| <= u / s: together (e_resize + u) / s + u / s = (10 + 2) u / s, taken at the
    smallest std.  Output type: ONE rounding of the fp32 value; the comparison allows one storage ulp of the largest binade the values reach -- values below
    R = 1 (plain) or R = max(m, 1 - m) / s (normalised) lie in binades up to 2^floor(log2 R) whose ulp is 2^(floor(log2 R) - 10) in fp16 and 2^(floor(log2 R) - 7) in
    bf16 (for R = 1: the 2^-11 / 2^-8 of _tta_cases).  Nothing here is fitted to what the kernel gives."""
    u = 2.0 ** -24
    if mean is None:
        tol, top = _tta_cases.scale_tolerance("f32"), -1          # values < 1: the largest binade is [0.5, 1)
    else:
        s = min(float(F32(v)) for v in std)
        r = max(max(float(F32(m)), 1.0 - float(F32(m))) / float(F32(sd)) for m, sd in zip(mean, std))
        tol, top = (_tta_cases.scale_tolerance("f32") + 2 * u) / s, math.floor(math.log2(r))
    return tol + {"f32": 0.0, "f16": 2.0 ** (top - 10), "bf16": 2.0 ** (top - 7)}[out_dt]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------------------
def image(h, w, in_dt, seed=0):
    """one image in its storage form: (3, h, w) of f32 / f16 / bf16 in [0, 1], (3, h, w) uint8, or (h, w, 3) uint8"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * h + w)
    if in_dt in ("u8", "u8hwc"):
        t = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
        return t.permute(1, 2, 0).contiguous() if in_dt == "u8hwc" else t
    return torch.rand(3, h, w, generator=g).to(TORCH_DT[in_dt])


def random_boxes(h, w, m, seed):
    """m boxes of a few pixels each, some across an edge"""
    g = np.random.default_rng(seed + 31 * h + w)
    x1, y1 = g.uniform(-4, w * 0.8, m), g.uniform(-4, h * 0.8, m)
    return np.stack([x1, y1, x1 + g.uniform(1, w * 0.6, m), y1 + g.uniform(1, h * 0.6, m)], 1).astype(F32)


class Case:
    """sizes: [(h, w)] per image; boxes: (n, K, 4) fp32 (slots at or past a count hold a sentinel that must never be read as a box); counts: per image, as handed in"""

    def __init__(self, name, sizes, counts, size, boxes=None, in_dt="f32", out_dt="f32", gain=1.02, pad=10, square=False, mean=None, std=None, cap=None, exact=False, seed=0):
        self.name, self.sizes, self.counts, self.size, self.in_dt, self.out_dt = name, list(sizes), list(counts), tuple(size), in_dt, out_dt
        self.gain, self.pad, self.square, self.mean, self.std, self.exact = gain, pad, square, mean, std, exact
        n = len(self.sizes)
        self.boxes = np.full((n, K, 4), 1.0e9, F32)
        for i, (h, w) in enumerate(self.sizes):
            c = min(max(self.counts[i], 0), K)
            if c:
                self.boxes[i, :c] = random_boxes(h, w, c, seed + i) if boxes is None else np.asarray(boxes[i], F32).reshape(-1, 4)[:c]
        self.images = [image(h, w, in_dt, seed + i) for i, (h, w) in enumerate(self.sizes)]
        self.clamped = [min(max(c, 0), K) for c in self.counts]
        self.total = sum(self.clamped)
        self.cap = self.total if cap is None else cap

    def expected_index(self):
        """(total, 6) int64 rows {image, detection, x1, y1, x2, y2}, image-major in slab order"""
        rows = []
        for i, (h, w) in enumerate(self.sizes):
            r = rect_ref(self.boxes[i, : self.clamped[i]], h, w, self.gain, self.pad, self.square)
            rows += [[i, j] + r[j].tolist() for j in range(self.clamped[i])]
        return torch.tensor(rows, dtype=torch.int64).reshape(-1, 6)

    def expected_status(self):
        return (STATUS_CAPACITY if self.total > self.cap else 0) | (STATUS_BAD_COUNT if self.clamped != self.counts else 0)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------------------------
def describe(case, images, boxes, counts, crops_ptr, index_ptr, total_ptr, keep):
    from yolort_amd._lib import CropDesc
    n = len(case.sizes)
    d = CropDesc()
    ptrs = (C.c_void_p * max(n, 1))(*[im.data_ptr() for im in images])
    hw = (C.c_int32 * max(2 * n, 1))(*[v for s in case.sizes for v in s])
    keep += [ptrs, hw]
    d.imgs, d.hw = C.cast(ptrs, C.POINTER(C.c_void_p)), C.cast(hw, C.POINTER(C.c_int32))
    d.boxes, d.counts, d.crops, d.index, d.total = boxes.data_ptr(), counts.data_ptr(), crops_ptr, index_ptr, total_ptr
    d.gain, d.pad, d.square, d.normalize = case.gain, case.pad, int(case.square), int(case.mean is not None)
    for i in range(3):
        d.mean[i], d.std[i] = (case.mean[i], case.std[i]) if case.mean is not None else (0.0, 1.0)
    d.n, d.k, d.cap, d.out_h, d.out_w = n, K, case.cap, case.size[0], case.size[1]
    d.in_dtype, d.out_dtype = DT_CODE[case.in_dt], DT_CODE[case.out_dt]
    return d


def error_text(lib):
    err = getattr(lib, "sim_last_error", None) or lib.ymi_last_error
    err.restype = C.c_char_p
    return err().decode()


def run_crop(lib, case, device="cpu", stream=None, slack=2):
    """ymi_crop_resize of `case` into poisoned buffers: the crops lie between two guard bands of a crop each and have `slack` rows of capacity-plus (rows the call must
    not touch either: the descriptor says case.cap), the index likewise.  -> dict(crops (cap + slack, 3, oh, ow) fp32, index (cap + slack, 6), total (2,), guards)"""
    lib.ymi_crop_resize.restype = C.c_int
    oh, ow = case.size
    tdt = TORCH_DT[case.out_dt]
    per = 3 * oh * ow
    band = (per + 7) // 8 * 8                                   # a multiple of 16 bytes: the body keeps the alignment of the allocation
    rows = case.cap + slack
    flat = torch.full((band + rows * per + band,), GUARD, dtype=tdt)
    idx = torch.full((6 + rows * 6 + 6,), int(GUARD), dtype=torch.int32)
    total = torch.full((4,), int(GUARD), dtype=torch.int32)
    images = [im.to(device) for im in case.images]
    boxes, counts = torch.from_numpy(case.boxes).to(device), torch.tensor(case.counts, dtype=torch.int32).to(device)
    flat, idx, total = flat.to(device), idx.to(device), total.to(device)
    keep = []
    d = describe(case, images, boxes, counts, flat.data_ptr() + band * flat.element_size(), idx.data_ptr() + 6 * 4, total.data_ptr() + 4, keep)
    rc = lib.ymi_crop_resize(C.byref(d), stream)
    assert rc == 0, (rc, error_text(lib))
    if device != "cpu":
        torch.cuda.synchronize()
    flat, idx, total = flat.cpu(), idx.cpu(), total.cpu()
    return dict(crops=flat[band: band + rows * per].view(rows, 3, oh, ow).float(), index=idx[6: 6 + rows * 6].view(rows, 6), total=total[1:3],
                guards=(flat[:band].float(), flat[-band:].float(), idx[:6], idx[-6:], total[0], total[3]))


def check_crop(out, case):
    """every comparison of one case: total and status, the index rows, the pixels (bit for bit where case.exact, within pixel_tolerance elsewhere), rows at or beyond the
    total and every guard band still poisoned.  -> the largest pixel error"""
    g = out["guards"]
    assert (g[0] == GUARD).all() and (g[1] == GUARD).all(), f"{case.name}: something outside the crops buffer was written"
    assert (g[2] == int(GUARD)).all() and (g[3] == int(GUARD)).all(), f"{case.name}: something outside the index buffer was written"
    assert int(g[4]) == int(GUARD) and int(g[5]) == int(GUARD), f"{case.name}: something around total[] was written"
    written = min(case.total, case.cap)
    assert out["total"].tolist() == [written, case.expected_status()], (case.name, out["total"].tolist(), written, case.expected_status())
    assert (out["crops"][written:] == GUARD).all(), f"{case.name}: a crop row at or beyond the total was written"
    assert (out["index"][written:] == int(GUARD)).all(), f"{case.name}: an index row at or beyond the total was written"
    want = case.expected_index()
    assert torch.equal(out["index"][:written].long(), want[:written]), (case.name, out["index"][:written].tolist(), want[:written].tolist())
    tol, worst = pixel_tolerance(case.out_dt, case.mean, case.std), 0.0
    wide = [widen(im, case.in_dt) for im in case.images]
    for row in range(written):
        i, _, *rect = want[row].tolist()
        got = out["crops"][row]
        if case.exact:
            ref = crop_ref_fp32(wide[i], rect, case.size, case.mean, case.std).to(TORCH_DT[case.out_dt]).float()
            assert torch.equal(got, ref), f"{case.name} row {row} rect {rect}: not bit for bit, max |diff| {float((got - ref).abs().max()):.3e}"
        else:
            ref = crop_ref(wide[i], rect, case.size, case.mean, case.std)
            err = float((got.double() - ref).abs().max())
            worst = max(worst, err)
            assert err <= tol, f"{case.name} row {row} rect {rect}: max |err| {err:.3e} > {tol:.3e}"
        if is_empty(rect):
            assert (got == 0).all(), f"{case.name} row {row}: an empty rectangle gives an all-zero crop"
    print(f"{case.name}: {written} crops, max |err| {worst:.3e} (tolerance {tol:.3e})")
    return worst


# ---- the case tables -----------------------------------------------------------------------------------------------------------------------------------------------
RAGGED_SIZES = [(48, 64), (37, 53), (8, 8), (48, 64), (37, 53), (8, 8)]
RAGGED_COUNTS = [0, 3, 0, 4, 2, 0]             # 0 for the first, a middle and the last image


def ragged(size, **kw):
    return Case(f"ragged-{size[0]}x{size[1]}-" + "-".join(f"{k}={v}" for k, v in kw.items() if k not in ("mean", "std")), RAGGED_SIZES, RAGGED_COUNTS, size, **kw)


def exact_boxes(size, h, w):
    """with gain 1 and pad 0: one rectangle of exactly (2 out_h, 2 out_w) (every weight 0.5), one of exactly (out_h, out_w) (the identity), both at odd offsets"""
    oh, ow = size
    assert 2 * oh + 3 <= h and 2 * ow + 5 <= w, (size, h, w)
    return [[5.0, 3.0, 5.0 + 2 * ow, 3.0 + 2 * oh], [3.0, 1.0, 3.0 + ow, 1.0 + oh]]


def exact_case(size, in_dt="f32", out_dt="f32", mean=None, std=None):
    sizes = [(48, 64), (37, 53)]
    return Case(f"exact-{size[0]}x{size[1]}-{in_dt}-{out_dt}" + ("-norm" if mean else ""), sizes, [2, 2], size, boxes=[exact_boxes(size, h, w) for h, w in sizes],
                in_dt=in_dt, out_dt=out_dt, gain=1.0, pad=0, mean=mean, std=std, exact=True)


def scaling_case(out_dt="f32"):
    """up-scaling a 3 x 2 rectangle (3 rows, 2 columns) to 16 x 12 -- the second tap must stop at the RECTANGLE's last row / column --, a 1 x 1 rectangle, and
    down-scaling most of the image to the same size"""
    boxes = [[[10.0, 5.0, 12.0, 8.0], [20.0, 30.0, 21.0, 31.0], [1.0, 2.0, 62.0, 45.0], [0.0, 0.0, 64.0, 48.0]]]
    return Case(f"scaling-{out_dt}", [(48, 64)], [4], (16, 12), boxes=boxes, out_dt=out_dt, gain=1.0, pad=0)


def many_images_case(size=(8, 8)):
    """66 images of 8 x 8: two launches (64 + 2 images); the rows of images 64 and 65 come after those of the first launch only if the offsets are global"""
    n = 66
    return Case(f"66-images-{size[0]}x{size[1]}", [(8, 8)] * n, [(i * 7 + 1) % 4 if i not in (0, 33, 65) else (0, 0, 3)[(0, 33, 65).index(i)] for i in range(n)], size, seed=5)


def nonfinite_case():
    nan, inf = float("nan"), float("inf")
    boxes = [[[nan, 2.0, 9.0, 9.0], [2.0, 2.0, inf, 9.0], [-inf, -inf, inf, inf], [4.0, 4.0, 20.0, 20.0]],
             [[-3.0e38, 2.0, 3.0e38, 9.0], [2.0, 3.0, 9.0, nan], [3.0, 3.0, 12.0, 14.0], [2.0, -inf, 9.0, 9.0]]]   # -3e38 .. 3e38: finite coordinates, an infinite width
    return Case("non-finite", [(48, 64), (37, 53)], [4, 4], (8, 8), boxes=boxes)


def golden_case(group, size=(7, 5)):
    """the boxes of one golden group as a slab: ceil(m / K) images of the group's size, every one the same picture"""
    b = np.asarray(group["boxes"], F32)
    m = len(b)
    n = (m + K - 1) // K
    counts = [min(K, m - i * K) for i in range(n)]
    boxes = [b[i * K: i * K + counts[i]] for i in range(n)]
    return Case(f"golden-{group['h']}x{group['w']}-g{group['gain']}-p{group['pad']}-{'square' if group['square'] else 'plain'}", [(group["h"], group["w"])] * n, counts, size,
                boxes=boxes, gain=group["gain"], pad=group["pad"], square=group["square"])


def refusals(base):
    """(what, change(d) applied to a valid descriptor, a word of the message) for every refusal of ymi_crop_resize"""
    nan, inf = float("nan"), float("inf")

    def setter(**kw):
        def f(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return f

    def std_zero(d):
        d.normalize, d.std[1] = 1, 0.0

    out = [(f"null {f}", setter(**{f: None}), "null") for f in ("imgs", "hw", "boxes", "counts", "crops", "index", "total")]
    out += [("out_h 0", setter(out_h=0), "below 1"), ("out_w -1", setter(out_w=-1), "below 1"), ("cap -1", setter(cap=-1), "capacity"),
            ("in_dtype 5", setter(in_dtype=5), "in_dtype"), ("in_dtype -1", setter(in_dtype=-1), "in_dtype"), ("out_dtype u8", setter(out_dtype=3), "out_dtype"),
            ("out_dtype 7", setter(out_dtype=7), "out_dtype"), ("std 0", std_zero, "std"), ("gain nan", setter(gain=nan), "finite"), ("gain inf", setter(gain=inf), "finite"),
            ("pad -inf", setter(pad=-inf), "finite"), ("pad nan", setter(pad=nan), "finite")]
    return out


def check_refusals(lib, device="cpu"):
    """every refusal returns YMI_EINVAL with a message and writes nothing"""
    case = ragged((8, 8))
    oh, ow = case.size
    crops = torch.full((case.cap, 3, oh, ow), GUARD).to(device)
    index = torch.full((case.cap, 6), int(GUARD), dtype=torch.int32).to(device)
    total = torch.full((2,), int(GUARD), dtype=torch.int32).to(device)
    images = [im.to(device) for im in case.images]
    boxes, counts = torch.from_numpy(case.boxes).to(device), torch.tensor(case.counts, dtype=torch.int32).to(device)
    lib.ymi_crop_resize.restype = C.c_int
    assert lib.ymi_crop_resize(None, None) == -1
    for what, change, word in refusals(case):
        keep = []
        d = describe(case, images, boxes, counts, crops.data_ptr(), index.data_ptr(), total.data_ptr(), keep)
        change(d)
        rc = lib.ymi_crop_resize(C.byref(d), None)
        assert rc == -1 and word in error_text(lib), (what, rc, error_text(lib))
    keep = []
    d = describe(case, images, boxes, counts, crops.data_ptr(), index.data_ptr(), total.data_ptr(), keep)
    null_image = (C.c_void_p * len(images))(*[im.data_ptr() for im in images])
    null_image[2] = None
    d.imgs = C.cast(null_image, C.POINTER(C.c_void_p))
    assert lib.ymi_crop_resize(C.byref(d), None) == -1 and "image 2" in error_text(lib)
    if device != "cpu":
        torch.cuda.synchronize()
    assert (crops.cpu() == GUARD).all() and (index.cpu() == int(GUARD)).all() and (total.cpu() == int(GUARD)).all(), "a refused call wrote something"
