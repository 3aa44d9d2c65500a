"""Shared by tests/test_nv12.py (the kernels of csrc/preproc_nv12.hip on the simulator) and tests/test_nv12_gpu.py (the real kernels): the NumPy restatements of the
NV12 conversion contract (include/yolort_amd.h), the case table and ONE driver of ymi_letterbox_nv12 -- the simulator takes host pointers, libyolort_amd.so device
pointers.  Yardsticks: `convert_int` (int64, the integer rule: compared bit for bit), `convert_real` (float64, the real-valued formula: within CONVERT_BOUND codes),
`model` = tests/_pre_cases.py's lb_resize(lb_widen(.)) of the converted frame rounded once (bit for bit), `ref64` (float64 end to end)."""
import ctypes as C
import functools
from typing import NamedTuple, Tuple

import numpy as np
import torch

from _pre_cases import DT_CODE, F32, FILL, LB_VARIANTS, TORCH_DT, Guarded, bits, env, lb_oracle_bound, lb_resize, lb_taps, lb_widen, place
from yolort_amd import _lib

TABLES = tuple((m, f) for m in ("bt601", "bt709") for f in (False, True))
CONVERT_BOUND = 0.5 + 495 * 2.0 ** -15      # rounding shift + (239 + 128 + 128) operand magnitudes x 2^-15 coefficient error
K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def _planes(y, uv):
    """(h, w) luma and (h / 2, w) interleaved chroma -> Y, Cb, Cr per pixel, nearest chroma"""
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)   # noqa: E731
    return y, up(uv[:, 0::2]), up(uv[:, 1::2])


def convert_int(y, uv, matrix, full):
    """the integer rule in int64 -> (h, w, 3) uint8"""
    cy, crv, cgu, cgv, cbu = _lib.NV12_COEF[(matrix, full)]
    l, cb, cr = (p.astype(np.int64) for p in _planes(y, uv))
    yc, cb, cr = (l - (0 if full else 16)) * cy + 8192, cb - 128, cr - 128
    return np.clip(np.stack([(yc + crv * cr) >> 14, (yc + cgu * cb + cgv * cr) >> 14, (yc + cbu * cb) >> 14], -1), 0, 255).astype(np.uint8)


def convert_real(y, uv, matrix, full):
    """the real-valued formula in float64, NOT clamped and not rounded -> (h, w, 3)"""
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    l, cb, cr = (p.astype(np.float64) for p in _planes(y, uv))
    l, cb, cr = (l, cb - 128, cr - 128) if full else ((l - 16) * 255 / 219, (cb - 128) * 255 / 224, (cr - 128) * 255 / 224)
    return np.stack([l + 2 * (1 - kr) * cr, l - 2 * kb * (1 - kb) / kg * cb - 2 * kr * (1 - kr) / kg * cr, l + 2 * (1 - kb) * cb], -1)


@functools.lru_cache(maxsize=None)
def grid_frame():
    """512 x 2048: every Y code against a 64 x 64 grid of (Cb, Cr) -> (y, uv).  Chroma pair p holds combination p % 4096; its four luma pixels hold 4 (p // 4096) + 0..3"""
    vals = np.unique(np.r_[0, 1, 127, 128, 129, 254, 255, np.round(np.linspace(3, 250, 57))]).astype(np.uint8)
    assert len(vals) == 64
    p = np.arange(256 * 1024).reshape(256, 1024)
    uv = np.empty((256, 2048), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = vals[p % 4096 // 64], vals[p % 64]
    y = (4 * np.repeat(np.repeat(p // 4096, 2, 0), 2, 1) + 2 * (np.arange(512) % 2)[:, None] + np.arange(2048) % 2).astype(np.uint8)
    return y, uv


class NvCase(NamedTuple):
    name: str
    out_dt: str
    frames: Tuple[Tuple[int, ...], ...]   # per frame (hin, win, hr, wr, pad_top, pad_left, pitch_y, pitch_uv, Y base offset, CbCr base offset past a 16-byte boundary)
    hb: int = 17
    wb: int = 130                         # 17 x 130: the last tile of every rows-per-wave / column-group value is ragged
    c_out: int = 4
    matrix: str = "bt601"
    full: bool = False


def _fr(hin, win, hr, wr, pt=0, pl=0, py=None, puv=None, oy=0, ouv=0):
    return (hin, win, hr, wr, pt, pl, py or win, puv or win, oy, ouv)


_MIS = tuple(_fr(6 + 2 * (i % 3), 18 + 16 * (i % 2), 7 + i, 40 + 9 * i, i % 3, i, 50, 48 + 2 * (i % 2), oy, ouv)
             for i, (oy, ouv) in enumerate(((0, 2), (1, 0), (5, 14), (8, 8), (15, 6), (4, 0), (11, 10), (3, 12))))
CASES = (
    NvCase("tiny", "f16", (_fr(2, 2, 8, 8, 1, 3), _fr(2, 4, 6, 12, 0, 118), _fr(4, 2, 12, 6, 5, 124), _fr(2, 2, 2, 2, 15, 127))),
    NvCase("scales", "f16", (_fr(10, 14, 17, 24, 0, 100), _fr(40, 38, 13, 12, 2, 118), _fr(16, 20, 16, 20, 1, 110), _fr(12, 40, 17, 57, 0, 73)), matrix="bt709"),
    NvCase("pitch", "bf16", (_fr(6, 18, 9, 27, 0, 0, 18, 18), _fr(6, 18, 9, 27, 1, 101, 48, 50), _fr(8, 34, 12, 51, 2, 79, 50, 48), _fr(8, 34, 5, 21, 3, 109, 48, 34)), full=True),
    NvCase("misaligned", "f32", _MIS, matrix="bt709", full=True),
    NvCase("cpr1", "f32", (_fr(8, 64, 16, 129),)),                      # columns 128.. of the canvas map to source column 63 alone: a tile of ONE staged chunk per row
    NvCase("n66", "f16", tuple(_fr(2 + 2 * (i % 3), 2 + 2 * (i % 5), 3 + i % 8, 4 + i % 13, i % 3, i % 5) for i in range(66)), 12, 20),   # a second launch
    NvCase("cout5", "bf16", (_fr(10, 14, 17, 24, 0, 100), _fr(40, 38, 13, 12, 2, 3)), c_out=5), NvCase("cout8", "f16", (_fr(10, 14, 17, 24, 0, 100),), c_out=8),
    NvCase("cout5-f32", "f32", (_fr(40, 38, 13, 12, 2, 3),), c_out=5),
    NvCase("stepdown", "f16", (_fr(68, 520, 17, 130), _fr(4, 6, 8, 12, 3, 60))),   # 4x down: rows-per-wave 4 and 2 exceed 64 KiB of LDS, 1 fits
    NvCase("up-f32", "f32", (_fr(10, 14, 17, 24, 0, 100),)), NvCase("down-f32", "f32", (_fr(40, 38, 13, 12, 2, 118),), matrix="bt709"),
)
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def frames(case):
    """random planes with their pitch: [(y (hin, pitch_y), uv (hin / 2, pitch_uv))] uint8; the first rows start with every code"""
    out = []
    for i, f in enumerate(case.frames):
        g = np.random.default_rng(100 + 7 * i + f[0] + f[1])
        out.append((g.integers(0, 256, (f[0], f[6]), dtype=np.uint8), g.integers(0, 256, (f[0] // 2, f[7]), dtype=np.uint8)))
    return out


def rgb8(case, i):
    (y, uv), f = frames(case)[i], case.frames[i]
    return convert_int(y[:, :f[1]], uv[:, :f[1]], case.matrix, case.full)


@functools.lru_cache(maxsize=None)
def model(case):
    """the expected canvas: the existing letterbox model on the converted frame, rounded once; pad pixels the fill, channels >= 3 zero"""
    out = np.zeros((len(case.frames), case.hb, case.wb, case.c_out), F32)
    out[..., :3] = F32(FILL)
    for i, (hin, win, hr, wr, pt, pl, *_) in enumerate(case.frames):
        out[i, pt: pt + hr, pl: pl + wr, :3] = lb_resize(lb_widen(torch.from_numpy(rgb8(case, i)), "u8hwc"), hr, wr).transpose(1, 2, 0)
    return torch.from_numpy(out).to(TORCH_DT[case.out_dt])


def ref64(case, i):
    """float64 end to end: the real-valued conversion clamped, / 255, bilinear with the same taps and weights -> (hr, wr, 3)"""
    (y, uv), (hin, win, hr, wr, *_) = frames(case)[i], case.frames[i]
    x = np.clip(convert_real(y[:, :win], uv[:, :win], case.matrix, case.full), 0, 255) / 255
    y0, y1, ly0, ly1 = lb_taps(hin, hr)
    x0, x1, lx0, lx1 = lb_taps(win, wr)
    lx0, lx1, ly0, ly1 = (w.astype(np.float64) for w in (lx0, lx1, ly0, ly1))
    top = x[y0][:, x0] * lx0[:, None] + x[y0][:, x1] * lx1[:, None]
    bot = x[y1][:, x0] * lx0[:, None] + x[y1][:, x1] * lx1[:, None]
    return top * ly0[:, None, None] + bot * ly1[:, None, None]


REF64_BOUND = CONVERT_BOUND / 255 + lb_oracle_bound()


def run(lib, case, variants=LB_VARIANTS, device="cpu", stream=None):
    """ymi_letterbox_nv12 of a case under every kernel variant, each into a poisoned destination between guard bands -> {variant: canvas on the host}"""
    n = len(case.frames)
    keep, d = [], _lib.Nv12Desc()
    ys, uvs = (C.c_void_p * n)(), (C.c_void_p * n)()
    for i, ((y, uv), f) in enumerate(zip(frames(case), case.frames)):
        for arr, ptrs, mis in ((y, ys, f[8]), (uv, uvs, f[9])):
            enc, ptrs[i] = place(torch.from_numpy(arr).reshape(-1), mis, device)
            keep.append(enc)
    pitch = (C.c_int32 * (2 * n))(*[v for f in case.frames for v in f[6:8]])
    geom = (C.c_int32 * (6 * n))(*[v for f in case.frames for v in f[:6]])
    d.y, d.uv, d.pitch, d.geom = C.cast(ys, C.POINTER(C.c_void_p)), C.cast(uvs, C.POINTER(C.c_void_p)), C.cast(pitch, C.POINTER(C.c_int32)), C.cast(geom, C.POINTER(C.c_int32))
    d.n, d.matrix, d.range = n, _lib.NV12_MATRIX[case.matrix], int(case.full)
    d.hb, d.wb, d.c_out, d.out_dtype, d.fill = case.hb, case.wb, case.c_out, DT_CODE[case.out_dt], FILL
    outs = {}
    for name, knob, cg in variants:
        dst = Guarded((n, case.hb, case.wb, case.c_out), case.wb * case.c_out, TORCH_DT[case.out_dt], device)
        d.out = dst.ptr
        with env(YOLORT_AMD_LETTERBOX=knob, YOLORT_AMD_LB_CG=cg):
            rc = lib.ymi_letterbox_nv12(C.byref(d), stream)
        assert rc == 0, (getattr(lib, "sim_last_error", None) or lib.ymi_last_error)()
        outs[name] = dst.read()
    return outs


def check(lib, case, device="cpu", variants=LB_VARIANTS):
    """every variant equals the model on raw bits (pad pixels and the zero channels are part of the model); the fp32 yardstick cases also against float64"""
    want = model(case)
    outs = run(lib, case, variants, device)
    for name, got in outs.items():
        diff = bits(got) != bits(want)
        assert not diff.any(), f"{case.name} [{name}]: {int(diff.sum())} elements differ from the model, first at (frame, y, x, c) = {tuple(int(v) for v in diff.nonzero()[0])}"
        if case.name in ("up-f32", "down-f32"):
            hin, win, hr, wr, pt, pl, *_ = case.frames[0]
            err = np.abs(got[0, pt: pt + hr, pl: pl + wr, :3].double().numpy() - ref64(case, 0)).max()
            print(f"{case.name} [{name}]: max |canvas - float64 reference| = {err:.3e}, bound {REF64_BOUND:.3e}")
            assert err <= REF64_BOUND
    return outs


def check_refusals(lib, device):
    """every YMI_EINVAL of the two entry points, each with its message; nothing is launched (the destination keeps its poison)"""
    y, uv = torch.zeros(8 * 16, dtype=torch.uint8).to(device), torch.zeros(4 * 16 + 1, dtype=torch.uint8).to(device)
    dst = Guarded((1, 8, 16, 4), 64, torch.float16, device)
    err = getattr(lib, "sim_last_error", None) or lib.ymi_last_error
    good = dict(h=8, w=16, py=16, puv=16, uv_off=0, matrix=0, range=0, out_dtype=0, c_out=4)
    bad = (dict(h=7), dict(w=15), dict(h=0), dict(w=1, py=2, puv=2), dict(py=17), dict(py=14), dict(puv=14), dict(puv=15), dict(uv_off=1), dict(matrix=2), dict(range=-1),
           dict(out_dtype=3), dict(c_out=2))
    for change in bad:
        a = dict(good, **change)
        d = _lib.Nv12Desc()
        ys, uvs = (C.c_void_p * 1)(y.data_ptr()), (C.c_void_p * 1)(uv.data_ptr() + a["uv_off"])
        pitch, geom = (C.c_int32 * 2)(a["py"], a["puv"]), (C.c_int32 * 6)(a["h"], a["w"], 8, 16, 0, 0)
        d.y, d.uv, d.pitch, d.geom = C.cast(ys, C.POINTER(C.c_void_p)), C.cast(uvs, C.POINTER(C.c_void_p)), C.cast(pitch, C.POINTER(C.c_int32)), C.cast(geom, C.POINTER(C.c_int32))
        d.n, d.matrix, d.range, d.out, d.hb, d.wb, d.c_out, d.out_dtype, d.fill = 1, a["matrix"], a["range"], dst.ptr, 8, 16, a["c_out"], a["out_dtype"], FILL
        assert lib.ymi_letterbox_nv12(C.byref(d), None) == -1 and b"ymi_letterbox_nv12" in err(), change
        if "out_dtype" not in change and "c_out" not in change:
            rgb = torch.zeros(8 * 16 * 3, dtype=torch.uint8).to(device)
            rc = lib.ymi_nv12_to_rgb(y.data_ptr(), uv.data_ptr() + a["uv_off"], a["py"], a["puv"], a["h"], a["w"], a["matrix"], a["range"], rgb.data_ptr(), None)
            assert rc == -1 and b"ymi_nv12_to_rgb" in err() and not rgb.any().item(), change
    assert torch.equal(bits(dst.read()), bits(dst.initial()))
