"""Shared by tests/test_pre_exact.py (CPU: the kernels of csrc/preproc_pool.hip on the simulator, the non-vacuity checks, the letterbox model held to the oracle) and
tests/test_pre_exact_gpu.py (the real kernels): the case tables, the references and ONE driver per entry point -- the simulator takes host pointers, libyolort_amd.so
device pointers, the calls are the same (ymi_letterbox, ymi_spp_pool, ymi_upsample2x, ymi_copy_view, ymi_nchw_to_nhwc, ymi_nhwc_to_nchw through the prototypes of
yolort_amd/_lib.py).  Every driver poisons its destination, places it between two guard bands of at least a row each and asserts that the bands and every channel
outside the addressed slice keep their bits.

Yardsticks
  letterbox   `lb_model`: a NumPy float32 model of the kernel's stated arithmetic (nested, unfused lerp), compared BIT FOR BIT with every kernel variant; the model itself
              is held to the oracle's letterbox within `lb_oracle_bound` (tests/test_pre_exact.py)
  SPP         F.max_pool2d(x.float(), k, 1, k // 2), k = 5 / 9 / 13, bit for bit after narrowing (a zero of either sign where the reference is a zero)
  upsample    F.interpolate(scale_factor=2, mode="nearest") (of the pixel INDEX: the kernels are typeless copies and the cases hold NaN patterns), raw bits
  view copy   plain slicing, raw bits
  layout      permute + .to(dtype) on the CPU (round to nearest even), raw bits

Which case reaches which kernel of csrc/preproc_pool.hip (scale_view_kernel, crop_resize_kernel, act_kernel and act_f32_kernel have files of their own):
  kernel, template variant                     case(s)                                     dispatch condition (host code of the same file)
  letterbox_kernel<IDT, ODT>                   every LB case under variant pixel-cg*;      YOLORT_AMD_LETTERBOX=pixel; or c_out != 4; or no rows-per-wave value whose
    IDT 5 types x ODT 3 types                  cout5-*, cout8-*; fallback-f32 (default)    staged rows fit 64 KiB (letterbox_tile_lds == 0 for rpw 4, 2 and 1)
  letterbox_tile2_kernel<IDT, ODT, RPW, CG>    io-*, up-*, down3-*, one-*, cpr1-*,         c_out == 4, not every image at its resized size or wb % 4 != 0; RPW = the
    RPW 4 / 2 / 1 x CG 1 / 2                   edge-*, mis-*, w161-*, w162-*, n66-*        largest of YOLORT_AMD_LETTERBOX (default 4), halved until the rows fit;
                                               under variants 1-cg*, 2-cg*, 4-cg*, default CG = YOLORT_AMD_LB_CG (default 1; 2 falls back to 1 when it does not fit)
  letterbox_copy_kernel<IDT, ODT, 8>           copy160-*                                   c_out == 4, wb % 8 == 0, every image has hin == hr and win == wr
  letterbox_copy_kernel<IDT, ODT, 4>           copy164-*                                   the same with wb % 8 == 4
  nchw_to_nhwc_kernel<IDT, ODT> (7 pairs)      LAYOUT_PAIRS x LAYOUT_MAPS, c_pad 4 and 8   always (ymi_nchw_to_nhwc)
  nhwc_to_nchw_kernel<IDT, ODT> (7 pairs)      LAYOUT_PAIRS x LAYOUT_MAPS, c = 3 and 16    always (ymi_nhwc_to_nchw)
  spp_pool_lds_kernel<F16 / BF16, 4>           auto-c32, force-g4, fit-g4,                 c % 32 == 0 and h * w * 4 * 32 <= 160 KiB - 512; YOLORT_AMD_SPP_G=4
                                               nt-256 / 512 / 1024
  spp_pool_lds_kernel<F16 / BF16, 2>           auto-c16, auto-c48, force-g2, miss-g4,      c % 16 == 0 (and not % 32), or G = 4 does not fit; YOLORT_AMD_SPP_G=2
                                               fit-g2
  spp_pool_lds_kernel<F16 / BF16, 1>           auto-c8, auto-c24, auto-c40, force-g1,      c % 16 != 0, or G = 2 does not fit; YOLORT_AMD_SPP_G=1
                                               miss-g2, fit-g1, small-*
  spp_pool_kernel<F16 / BF16>                  direct (70 x 73, c = 8)                     h * w * 32 > 160 KiB - 512 (G = 1 does not fit)
  spp_pool_f32_lds_kernel                      fit-g1 (f32), auto-c8 (f32), small-* (f32)  dtype F32 and h * w * 32 <= 160 KiB - 512
  spp_pool_f32_kernel                          direct (f32, 70 x 73, c = 8)                dtype F32 and the plane does not fit
  upsample2x_kernel                            UP_MAPS x f16 / bf16 / f32                  always (ymi_upsample2x; fp32 counted in 2-byte units)
  copy_view_kernel                             UP_MAPS x f16 / bf16 / f32                  always (ymi_copy_view)
"""
import contextlib
import ctypes as C
import functools
import os
from typing import NamedTuple, Tuple

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
GUARD = -7.0                                       # poison of every destination and of its guard bands
YMI_OK, YMI_EINVAL = 0, -1
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "u8": torch.uint8, "u8hwc": torch.uint8}
DT_CODE = {"f16": 0, "bf16": 1, "f32": 2, "u8": 3, "u8hwc": 4}
ESZ = {"f16": 2, "bf16": 2, "f32": 4, "u8": 1, "u8hwc": 1}
IN_DTS, OUT_DTS = ("f32", "f16", "bf16", "u8", "u8hwc"), ("f16", "bf16", "f32")
ENTRIES = ("ymi_letterbox", "ymi_spp_pool", "ymi_upsample2x", "ymi_copy_view", "ymi_nchw_to_nhwc", "ymi_nhwc_to_nchw")
FILL = 114.0 / 255.0
LB_MAX, LB_TW, LB_LDS_CAP = 64, 128, 64 * 1024     # images per launch, columns per tile group, the largest dynamic LDS request that needs no opt-in
SPP_LDS, SPP_BLOCK_BYTES = 160 * 1024 - 512, 32    # the LDS budget of the cascade kernels; bytes per pixel and 8-channel group (the plane twice, 16 bytes each)


def proto(lib):
    """the prototypes of yolort_amd/_lib.py on the six entry points of `lib` (the simulator library exports them under the same names)"""
    from yolort_amd._lib import _SIGS
    for name in ENTRIES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _SIGS[name]
    return lib


def last_error(lib):
    err = getattr(lib, "sim_last_error", None) or lib.ymi_last_error
    err.restype = C.c_char_p
    return err().decode()


@contextlib.contextmanager
def env(**kv):
    """environment variables for the duration of a call (the host wrappers read them per call); None removes one"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bits(t):
    """the raw bits of a tensor as integers (NaN patterns and signed zeros compare as what they are)"""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _sync(device):
    if str(device) != "cpu":
        torch.cuda.synchronize()


class Guarded:
    """a poisoned destination of `shape` between two guard bands of at least `row` elements each (rounded up to 64 elements, so the body keeps the 16-byte alignment
    the allocator gives); `fill` = initial body (default: poison everywhere)"""

    def __init__(self, shape, row, tdt, device, fill=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.band = (max(int(row), 1) + 63) // 64 * 64
        flat = torch.full((2 * self.band + self.n,), GUARD if tdt.is_floating_point else 0x7BAD, dtype=tdt)
        if fill is not None:
            flat[self.band: self.band + self.n] = fill.reshape(-1)
        self.before, self.dev, self.device = flat, flat.to(device), device
        assert self.ptr % 16 == 0

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.band * self.dev.element_size()

    def initial(self):
        return self.before[self.band: self.band + self.n].view(self.shape)

    def read(self):
        """-> the body on the host, after asserting that both guard bands kept their bits"""
        _sync(self.device)
        flat = self.dev.cpu()
        assert torch.equal(bits(flat[:self.band]), bits(self.before[:self.band])), "the guard band before the destination was written"
        assert torch.equal(bits(flat[self.band + self.n:]), bits(self.before[self.band + self.n:])), "the guard band after the destination was written"
        return flat[self.band: self.band + self.n].view(self.shape)


# ---- 1. letterbox --------------------------------------------------------------------------------------------------------------------------------------------------
LB_VARIANTS = (("default", None, None),) + tuple((f"{k}-cg{cg}", k, cg) for k in ("pixel", "1", "2", "4") for cg in ("1", "2"))


class LbCase(NamedTuple):
    name: str
    in_dt: str
    out_dt: str
    geoms: Tuple[Tuple[int, int, int, int, int, int], ...]   # per image (hin, win, hr, wr, pad_top, pad_left)
    hb: int
    wb: int
    c_out: int = 4
    mis: Tuple[int, ...] = ()                                # per image: bytes of its base pointer past a 16-byte boundary (default 0)

    def misalign(self, i):
        return self.mis[i] if self.mis else 0


def lb_bpp(in_dt):
    return 3 if in_dt == "u8hwc" else ESZ[in_dt]


def lb_image(in_dt, hin, win, seed):
    """random pixels already rounded to the input type: (3, hin, win), or (hin, win, 3) uint8 for the interleaved type.  A uint8 image of at least 256 elements
    starts with all 256 values"""
    g = torch.Generator().manual_seed(1000 + seed)
    if in_dt in ("u8", "u8hwc"):
        im = torch.randint(0, 256, (3, hin, win), generator=g, dtype=torch.uint8)
        if im.numel() >= 256:
            im.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
        return im.permute(1, 2, 0).contiguous() if in_dt == "u8hwc" else im
    return torch.rand(3, hin, win, generator=g).to(TORCH_DT[in_dt])


def lb_widen(im, in_dt):
    """the input widened exactly to float32 (3, hin, win); uint8: float32(v) / float32(255), one rounded division"""
    if in_dt == "u8hwc":
        im = im.permute(2, 0, 1)
    if in_dt in ("u8", "u8hwc"):
        return im.contiguous().numpy().astype(F32) / F32(255)
    return im.float().contiguous().numpy()


def lb_taps(n_in, n_out):
    """source taps of every destination index of one axis, in float32: scale = fl(n_in / n_out); coordinate fl(fl(scale * (d + 0.5)) - 0.5), clamped at 0 and
    truncated; both indices clamped at n_in - 1; the weight of the second tap clamped to [0, 1], the first one's is fl(1 - l1)"""
    s = F32(n_in) / F32(n_out)
    d = np.arange(n_out, dtype=F32)
    f = np.maximum((s * (d + F32(0.5))).astype(F32) - F32(0.5), F32(0))
    i0 = np.minimum(f.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = np.clip((f - i0.astype(F32)).astype(F32), F32(0), F32(1))
    l0 = (F32(1) - l1).astype(F32)
    assert f.dtype == l1.dtype == l0.dtype == F32
    return i0, i1, l0, l1


def lb_resize(x, hr, wr):
    """the resized image of the model, float32 (3, hr, wr): top, bot and the value are each two rounded products and one rounded sum (NumPy evaluates every
    operator of an expression on its own, in float32: nothing is fused)"""
    assert x.dtype == F32
    y0, y1, ly0, ly1 = lb_taps(x.shape[1], hr)
    x0, x1, lx0, lx1 = lb_taps(x.shape[2], wr)
    r0, r1 = x[:, y0], x[:, y1]
    top = r0[:, :, x0] * lx0 + r0[:, :, x1] * lx1
    bot = r1[:, :, x0] * lx0 + r1[:, :, x1] * lx1
    out = top * ly0[:, None] + bot * ly1[:, None]
    assert out.dtype == F32
    return out


@functools.lru_cache(maxsize=None)
def lb_images(case):
    return tuple(lb_image(case.in_dt, g[0], g[1], seed=17 * i + g[0] + g[1]) for i, g in enumerate(case.geoms))


@functools.lru_cache(maxsize=None)
def lb_model(case):
    """-> the expected canvas (n, hb, wb, c_out) in the output type: resized pixels of `lb_resize` rounded ONCE (to nearest even) to the output type, pad pixels the
    fill value rounded once, channels 3 and above exactly zero"""
    n = len(case.geoms)
    out = np.zeros((n, case.hb, case.wb, case.c_out), F32)
    out[..., :3] = F32(FILL)
    for i, ((hin, win, hr, wr, pt, pl), im) in enumerate(zip(case.geoms, lb_images(case))):
        out[i, pt: pt + hr, pl: pl + wr, :3] = lb_resize(lb_widen(im, case.in_dt), hr, wr).transpose(1, 2, 0)
    return torch.from_numpy(out).to(TORCH_DT[case.out_dt])


def place(raw, mis, device):
    """the bytes `raw` as a view into a larger tensor whose base sits `mis` bytes past a 16-byte boundary -> (enclosing tensor, pointer).  By construction the
    aligned 16-byte chunks that hold the first and the last byte lie inside the enclosing tensor; asserted"""
    nb = raw.numel()
    enc = torch.full((nb + 96,), 0xA5, dtype=torch.uint8).to(device)
    off = (-enc.data_ptr()) % 16 + 16 + mis
    enc[off: off + nb] = raw.to(device)
    ptr = enc.data_ptr() + off
    assert ptr % 16 == mis % 16
    assert enc.data_ptr() <= (ptr & ~15) and ((ptr + nb + 15) & ~15) <= enc.data_ptr() + enc.numel(), "the source view leaves its enclosing tensor"
    return enc, ptr


def run_letterbox(lib, case, variants=LB_VARIANTS, device="cpu", stream=None):
    """ymi_letterbox of a case under every kernel variant -> {variant name: canvas (n, hb, wb, c_out) on the host}"""
    n = len(case.geoms)
    keep, ptrs = [], (C.c_void_p * max(n, 1))()
    for i, im in enumerate(lb_images(case)):
        assert case.misalign(i) % ESZ[case.in_dt] == 0
        enc, ptr = place(bits(im).view(torch.uint8).reshape(-1), case.misalign(i), device)
        keep.append(enc)
        ptrs[i] = ptr
    geom = (C.c_int32 * max(6 * n, 1))(*[v for g in case.geoms for v in g])
    outs = {}
    for name, knob, cg in variants:
        dst = Guarded((n, case.hb, case.wb, case.c_out), case.wb * case.c_out, TORCH_DT[case.out_dt], device)
        with env(YOLORT_AMD_LETTERBOX=knob, YOLORT_AMD_LB_CG=cg, YOLORT_AMD_LB_DEBUG=None):
            rc = lib.ymi_letterbox(ptrs, geom, n, DT_CODE[case.in_dt], C.c_void_p(dst.ptr), case.hb, case.wb, case.c_out, DT_CODE[case.out_dt], C.c_float(FILL), stream)
        assert rc == YMI_OK, last_error(lib)
        outs[name] = dst.read()
    return outs


def check_letterbox(lib, case, device="cpu", variants=LB_VARIANTS):
    """every variant equals the model bit for bit; pad pixels = the fill value rounded once, channels >= 3 exactly zero, identity copies of a 16-bit type = the source bits"""
    want = lb_model(case)
    outs = run_letterbox(lib, case, variants, device)
    fill = torch.tensor(FILL, dtype=torch.float32).to(TORCH_DT[case.out_dt])
    for name, got in outs.items():
        assert got.shape == want.shape
        diff = bits(got) != bits(want)
        assert not diff.any(), f"{case.name} [{name}]: {int(diff.sum())} elements differ from the model, first at (img, y, x, c) = {tuple(int(v) for v in diff.nonzero()[0])}"
        assert (bits(got[..., 3:]) == 0).all(), f"{case.name} [{name}]: channel 3 and above must be +0"
        for i, (hin, win, hr, wr, pt, pl) in enumerate(case.geoms):
            pad = torch.ones(case.hb, case.wb, dtype=torch.bool)
            pad[pt: pt + hr, pl: pl + wr] = False
            assert (bits(got[i, ..., :3][pad]) == bits(fill.reshape(1))).all(), f"{case.name} [{name}]: pad pixels of image {i}"
            if (hin, win) == (hr, wr) and case.in_dt == case.out_dt and case.in_dt in ("f16", "bf16"):
                src = lb_images(case)[i].permute(1, 2, 0)
                assert torch.equal(bits(got[i, pt: pt + hr, pl: pl + wr, :3]), bits(src)), f"{case.name} [{name}]: an identity copy must keep the source bits"
    return outs


# -- what the host does with a case, restated from the geometry alone (non-vacuity checks) --
def lb_tile_lds(case, geoms, th, tw):
    """the dynamic LDS request of the tiled kernel for tiles of th x tw, by the host's formula; 0 = does not fit 64 KiB"""
    bpp, planes, need = lb_bpp(case.in_dt), (1 if case.in_dt == "u8hwc" else 3), 16
    for hin, win, hr, wr, _, _ in geoms:
        rows, cols = int(th * (hin / hr)) + 3, int(tw * (win / wr)) + 3
        pitch = ((min(cols, win) * bpp + 30) >> 4) << 4
        need = max(need, planes * min(rows, hin) * pitch)
    return need if need <= LB_LDS_CAP else 0


def lb_dispatch(case, knob=None, cg=None):
    """per launch (LB_MAX images each) the kernel the host picks: ("copy", px) | ("tile", rpw, cg) | ("pixel",)"""
    out = []
    for base in range(0, len(case.geoms), LB_MAX):
        geoms = case.geoms[base: base + LB_MAX]
        if case.c_out == 4 and case.wb % 4 == 0 and all((g[0], g[1]) == (g[2], g[3]) for g in geoms):
            out.append(("copy", 8 if case.wb % 8 == 0 else 4))
            continue
        pick = ("pixel",)
        if case.c_out == 4 and knob != "pixel":
            rpw = int(knob) if knob in ("1", "2", "4") else 4
            while rpw >= 1:
                for g_ in ((2, 1) if cg == "2" else (1,)):
                    if lb_tile_lds(case, geoms, 4 * rpw, LB_TW * g_):
                        pick = ("tile", rpw, g_)
                        break
                if pick[0] == "tile":
                    break
                rpw >>= 1
        out.append(pick)
    return out


def lb_tiles(case, rpw, cg):
    """every (image, tile) of a tiled launch that overlaps the resized region: dict(img, straddle = the tile also holds pad pixels, span = staged bytes per row,
    al_a = 16-byte misalignment of the first staged byte)"""
    th, tw, bpp, out = 4 * rpw, LB_TW * cg, lb_bpp(case.in_dt), []
    for i, (hin, win, hr, wr, pt, pl) in enumerate(case.geoms):
        x0, x1, _, _ = lb_taps(win, wr)
        for y0t in range(0, case.hb, th):
            for x0t in range(0, case.wb, tw):
                ya, yb = max(y0t, pt), min(y0t + th, pt + hr, case.hb)
                xa, xb = max(x0t, pl), min(x0t + tw, pl + wr, case.wb)
                if ya >= yb or xa >= xb:
                    continue
                cx0, cx1 = int(x0[xa - pl]), int(x1[xb - 1 - pl])
                full = (ya, yb, xa, xb) == (y0t, min(y0t + th, case.hb), x0t, min(x0t + tw, case.wb))
                out.append(dict(img=i, straddle=not full, span=(cx1 - cx0 + 1) * bpp, al_a=(case.misalign(i) + cx0 * bpp) % 16,
                                al_p=(hin * win * ESZ[case.in_dt]) % 16, al_r=(win * bpp) % 16))
    return out


def lb_oracle_bound():
    """|model - oracle| for pixels in [0, R], R = 1, in float32 (u = 2^-24).  Both sides take the source coordinate as fl(fl(scale * (d + 0.5)) - 0.5) and the weights
    as l1 = f - i0 (exact: f >= i0 share a binade or i0's is lower), l0 = fl(1 - l1), so the weights are the SAME float32 numbers and l0 + l1 <= 1 + u.  The nested form
    rounds, per row pair, two products (errors u * p00 * l0 + u * p01 * l1 <= u R) and their sum (u R): top and bot carry 2 u R each.  The vertical step scales these by
    ly0 + ly1 (<= 2 u R in all), adds two rounded products (u R together) and one rounded sum (u R): 4 u R against the exact bilinear value of the same weights, to
    first order in u.  The oracle's form (ATen's arithmetic restated in torch fp32 ops: the same expression, or the four-tap form with 5 roundings of partial sums <= R)
    is at most 5 u R off the same exact value, in the other direction at worst: 9 * 2^-24.  The oracle in this repository happens to evaluate the nested form in the
    same order with unfused torch ops, so the measured maximum is expected to be 0; the bound is what the counting guarantees without that coincidence."""
    return 9 * 2.0 ** -24


def _lb(name, in_dt, out_dt, geoms, hb, wb, c_out=4, mis=()):
    return LbCase(name, in_dt, out_dt, tuple(tuple(g) for g in geoms), hb, wb, c_out, tuple(mis))


_IO_GEOMS = ((23, 97, 31, 131, 1, 3), (40, 201, 20, 100, 5, 29), (32, 160, 32, 160, 0, 0))   # up 1.35x with odd pads; down 2.01x ending on column 128; an identity image
_MIS_GEOMS = tuple((21 + 2 * i, 95 + 2 * i, 24 + i, 120 + 5 * i, i % 3, 2 * i + 1) for i in range(6))   # row pitch and plane size are odd numbers of elements
_COPY_GEOMS = {160: ((32, 160, 32, 160, 0, 0), (20, 100, 20, 100, 3, 28), (17, 53, 17, 53, 7, 13), (30, 64, 30, 64, 1, 8), (9, 48, 9, 48, 20, 108)),
               164: ((32, 164, 32, 164, 0, 0), (20, 100, 20, 100, 3, 28), (17, 53, 17, 53, 7, 13), (10, 8, 10, 8, 0, 152), (9, 50, 9, 50, 20, 12))}
_N66 = tuple((3 + i % 7, 4 + i % 9, 8 + i % 20, 10 + (3 * i) % 19, i % 5, (2 * i) % 4) for i in range(66))

LB_CASES = tuple(
    # every input type x every output type: three images, so the image index matters
    [_lb(f"io-{i}-{o}", i, o, _IO_GEOMS, 32, 160) for i in IN_DTS for o in OUT_DTS] + [
        # up-scale 8x: 5 x 7 -> 40 x 56 across the tile boundary at column 128
        _lb("up-u8", "u8", "f16", [(5, 7, 40, 56, 3, 100)], 48, 160), _lb("up-f16", "f16", "f32", [(5, 7, 40, 56, 3, 100)], 48, 160),
        # down-scale 3x that still fits the tiled kernel's LDS (bf16: at two rows per wave)
        _lb("down3-bf16", "bf16", "bf16", [(95, 479, 31, 159, 0, 1)], 32, 160), _lb("down3-u8hwc", "u8hwc", "f16", [(95, 479, 31, 159, 0, 1)], 32, 160),
        # one image whose 6x down-scale does not fit at any rows-per-wave value: the whole launch takes the per-pixel kernel
        _lb("fallback-f32", "f32", "f32", [(20, 100, 25, 125, 2, 5), (30, 240, 5, 40, 20, 60)], 32, 160),
        # degenerate sizes, each alone
        _lb("one-win", "u8", "f16", [(9, 1, 18, 40, 2, 110)], 32, 160), _lb("one-hin", "f16", "f16", [(1, 50, 20, 100, 3, 40)], 32, 160),
        _lb("one-hr", "bf16", "f32", [(7, 90, 1, 130, 15, 10)], 32, 160), _lb("one-wr", "u8hwc", "bf16", [(20, 6, 30, 1, 1, 128)], 32, 160),
        # the three geometries whose last tile stages ONE uint8 source column (cpr == 1)
        _lb("cpr1-a", "u8", "f32", [(8, 65, 16, 129, 0, 0)], 32, 160), _lb("cpr1-b", "u8", "f32", [(9, 33, 27, 257, 3, 0)], 32, 288),
        _lb("cpr1-c", "u8", "f32", [(5, 40, 10, 125, 2, 4)], 32, 160),
        # a resized region that ends on the first / on the last column of a 128-column tile
        _lb("edge-first-col", "f16", "f16", [(40, 201, 20, 100, 5, 29)], 32, 160), _lb("edge-last-col", "u8", "bf16", [(30, 70, 28, 98, 3, 30)], 32, 160),
        # misaligned sources: views whose base sits `mis` bytes past a 16-byte boundary; odd row pitch and plane size
        _lb("mis-u8", "u8", "f16", _MIS_GEOMS, 32, 160, mis=(1, 2, 3, 5, 8, 15)), _lb("mis-u8hwc", "u8hwc", "f32", _MIS_GEOMS, 32, 160, mis=(1, 2, 3, 5, 8, 15)),
        _lb("mis-f16", "f16", "f16", _MIS_GEOMS[:3], 32, 160, mis=(2, 6, 14)), _lb("mis-bf16", "bf16", "f32", _MIS_GEOMS[3:], 32, 160, mis=(2, 6, 14)),
        _lb("mis-f32", "f32", "bf16", _MIS_GEOMS[1:3], 32, 160, mis=(4, 12)),
        # canvas width odd / even but no multiple of 4: identity sizes (the copy kernel refuses them: resampling kernels at scale 1) and a real resize
        _lb("w161-identity", "f16", "f16", [(32, 161, 32, 161, 0, 0), (20, 100, 20, 100, 7, 31)], 32, 161),
        _lb("w162-identity", "bf16", "bf16", [(32, 162, 32, 162, 0, 0), (20, 100, 20, 100, 7, 31)], 32, 162),
        _lb("w161-resize", "u8", "bf16", [(23, 97, 31, 131, 1, 3), (20, 50, 32, 161, 0, 0)], 32, 161),
        _lb("w162-resize", "u8hwc", "f32", [(23, 97, 31, 131, 1, 3), (20, 50, 32, 162, 0, 0)], 32, 162),
        _lb("w161-resize-f16", "f32", "f16", [(23, 97, 31, 131, 1, 3), (40, 201, 20, 100, 5, 61)], 33, 161),
        # c_out 8 and 5 (4 is everywhere else): the per-pixel kernel's 16-byte store and its scalar store loop
        _lb("cout8-f16", "f16", "f16", _IO_GEOMS, 32, 160, c_out=8), _lb("cout5-bf16", "u8", "bf16", _IO_GEOMS, 32, 160, c_out=5),
        _lb("cout5-f32", "f32", "f32", _IO_GEOMS, 32, 160, c_out=5),
        # 66 images of different geometry: two launches, the second at its output offset
        _lb("n66-f16", "u8", "f16", _N66, 32, 32), _lb("n66-f32", "f16", "f32", _N66, 32, 32),
        # no image at all
        _lb("empty", "f16", "f16", [], 32, 160),
    ] +
    # identity copy kernel, 8 and 4 pixels per thread: win and pad_left multiples of 8, of 4 only, of neither
    [_lb(f"copy{wb}-{i}-{o}", i, o, _COPY_GEOMS[wb], 32, wb) for wb in (160, 164)
     for i, o in (("f16", "f16"), ("bf16", "bf16"), ("f32", "f32"), ("u8", "f16"), ("u8hwc", "f32"), ("f16", "bf16"), ("bf16", "f32"), ("f32", "f16"))])
LB_BY_NAME = {c.name: c for c in LB_CASES}
assert len(LB_BY_NAME) == len(LB_CASES)


# ---- 2. SPP pyramid ---------------------------------------------------------------------------------------------------------------------------------------------------
class SppCase(NamedTuple):
    name: str
    h: int
    w: int
    c: int
    n: int = 3
    g: str = None          # YOLORT_AMD_SPP_G
    nt: str = None         # YOLORT_AMD_SPP_NT
    dts: Tuple[str, ...] = ("f16", "bf16")


def spp_fit(g):
    """the largest pixel count whose plane fits the LDS budget twice with g 8-channel groups per block"""
    return SPP_LDS // (g * SPP_BLOCK_BYTES)


def spp_path(case, dt):
    """the kernel the host picks: ("lds", G) | ("direct",) | ("lds32",) | ("direct32",)"""
    px = case.h * case.w
    if dt == "f32":
        return ("lds32",) if px <= spp_fit(1) else ("direct32",)
    g = 4 if case.c % 32 == 0 else (2 if case.c % 16 == 0 else 1)
    while g > 1 and px > spp_fit(g):
        g //= 2
    if case.g is not None and (int(case.g) == 1 or (int(case.g) == 2 and g >= 2) or (int(case.g) == 4 and g == 4)):
        g = int(case.g)
    return ("lds", g) if px <= spp_fit(g) else ("direct",)


SPP_CASES = tuple(
    [SppCase(f"auto-c{c}", 20, 17, c, dts=("f16", "bf16", "f32") if c == 8 else ("f16", "bf16")) for c in (32, 16, 48, 8, 24, 40)] +
    [SppCase(f"force-g{g}", 13, 21, 32, g=str(g)) for g in (1, 2, 4)] +
    [SppCase("fit-g4", 29, 44, 32, n=1), SppCase("miss-g4", 18, 71, 32, n=1), SppCase("fit-g2", 44, 58, 16, n=1), SppCase("miss-g2", 37, 69, 16, n=1),
     SppCase("fit-g1", 58, 88, 8, n=1, dts=("f16", "bf16", "f32")), SppCase("direct", 70, 73, 8, n=1, dts=("f16", "bf16", "f32"))] +
    [SppCase(f"small-{h}x{w}", h, w, 8, dts=("f16", "bf16", "f32")) for h, w in ((1, 1), (1, 7), (7, 1), (2, 3), (4, 4), (6, 13))] +
    [SppCase(f"nt-{nt}", 20, 20, 32, nt=str(nt)) for nt in (256, 512, 1024)])
SPP_BY_NAME = {c.name: c for c in SPP_CASES}
SPP_THRESHOLD_PAIRS = (("fit-g4", "miss-g4", 4), ("fit-g2", "miss-g2", 2), ("fit-g1", "direct", 1))   # (largest fit, first miss, G)
_SPP_LIMITS = {"f16": (2.0 ** -24, 1023, 65504.0, (1.0, 1e-3, 100.0, 1e4)), "bf16": (2.0 ** -133, 127, 3.3895313892515355e38, (1e-30, 1.0, 3e4, 1e30)),
               "f32": (2.0 ** -149, 2 ** 23 - 1, 3.4028234663852886e38, (1e-30, 1.0, 3e4, 1e30))}   # smallest subnormal, largest subnormal count, largest finite, magnitudes


@functools.lru_cache(maxsize=None)
def spp_input(dt, n, c, h, w):
    """(n, c, h, w) in the storage type, no NaN.  By channel % 8: 0 normal values, subnormals of both signs and zeros of both signs mixed; 1 an all-negative plane (with
    -inf and the most negative finite value); 2 a constant plane (another constant per image, one of them a negative subnormal); 3 small values and the maximum in a
    corner (another corner per image: the largest finite value, +inf); 4 subnormals of both signs down to the smallest, and zeros; 5 normal values with one each of
    +-inf and +-largest finite; 6 negative subnormals and -0 with a single +0; 7 the wide-magnitude recipe (one magnitude per channel)"""
    tiny, kmax, big, mags = _SPP_LIMITS[dt]
    g = torch.Generator().manual_seed(7 + 31 * h + w + 3 * c)
    x = torch.zeros(n, c, h, w, dtype=torch.float64)
    rnd = lambda: torch.randn(n, h, w, generator=g, dtype=torch.float64)   # noqa: E731
    uni = lambda: torch.rand(n, h, w, generator=g, dtype=torch.float64)    # noqa: E731
    sub = lambda: torch.randint(1, kmax + 1, (n, h, w), generator=g).double() * tiny   # noqa: E731
    sign = lambda: torch.where(uni() < 0.5, -1.0, 1.0)                     # noqa: E731
    corners = ((0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0))
    for ch in range(c):
        kind, p = ch % 8, uni()
        if kind == 0:
            v = torch.where(p < 0.4, sub() * sign(), rnd())
            v = torch.where((p >= 0.4) & (p < 0.5), 0.0 * sign(), v)
            v = torch.where((p >= 0.5) & (p < 0.55), tiny * sign(), v)
        elif kind == 1:
            v = -rnd().abs() - 1.0
            v = torch.where(p < 0.03, -float("inf"), torch.where(p < 0.06, -big, v))
        elif kind == 2:
            v = torch.stack([torch.full((h, w), [0.37109375, -3.0 * tiny, -2.5][i % 3], dtype=torch.float64) for i in range(n)])
        elif kind == 3:
            v = rnd() * 0.1
            for i in range(n):
                v[i][corners[(i + ch // 8) % 4]] = (big, float("inf"), 5.0)[i % 3]
        elif kind == 4:
            v = torch.where(p < 0.8, sub() * sign(), 0.0 * sign())
            v = torch.where(p < 0.1, tiny * sign(), v)
        elif kind == 5:
            v = rnd()
            for j, s in enumerate((float("inf"), -float("inf"), big, -big)):
                for i in range(n):
                    k = int(torch.randint(0, h * w, (1,), generator=g))
                    if (i + j) % 2 == 0:
                        v[i].view(-1)[k] = s
        elif kind == 6:
            v = torch.where(p < 0.7, -sub(), torch.full((n, h, w), -0.0, dtype=torch.float64))
            v[0].view(-1)[int(torch.randint(0, h * w, (1,), generator=g))] = 0.0
        else:
            v = (rnd() * mags[(ch // 8) % 4]).clamp(-big, big)
            v[0, h // 3: h // 3 + 3, w // 4: w // 4 + 5] = 0.0
            v[0, min(h // 3 + 1, h - 1), min(w // 4 + 1, w - 1)] = -0.0
        x[:, ch] = v
    x = x.to(torch.float32).to(TORCH_DT[dt])
    assert not torch.isnan(x.float()).any()
    return x


@functools.lru_cache(maxsize=None)
def spp_ref(dt, n, c, h, w):
    """the three pools of the stored values widened to fp32, narrowed again (exact: a maximum is one of its inputs)"""
    x = spp_input(dt, n, c, h, w).float()
    return tuple(F.max_pool2d(x, k, 1, k // 2).to(TORCH_DT[dt]) for k in (5, 9, 13))


def run_spp(lib, case, dt, device="cpu", stream=None):
    """ymi_spp_pool on a poisoned (n, h, w, 4c + 8) buffer whose first c channels hold the input -> the three output slices [(n, c, h, w)] in the storage type.  Asserts
    that the input slice, the channels beyond 4c and the guard bands keep their bits."""
    n, c, h, w = case.n, case.c, case.h, case.w
    cs, tdt = 4 * c + 8, TORCH_DT[dt]
    x = spp_input(dt, n, c, h, w)
    body = torch.full((n, h, w, cs), GUARD, dtype=tdt)
    body[..., :c] = x.permute(0, 2, 3, 1)
    buf = Guarded((n, h, w, cs), w * cs, tdt, device, fill=body)
    with env(YOLORT_AMD_SPP_G=case.g, YOLORT_AMD_SPP_NT=case.nt):
        rc = lib.ymi_spp_pool(C.c_void_p(buf.ptr), n, h, w, c, cs, DT_CODE[dt], stream)
    assert rc == YMI_OK, last_error(lib)
    got = buf.read()
    assert torch.equal(bits(got[..., :c]), bits(body[..., :c])), "the input slice was changed"
    assert torch.equal(bits(got[..., 4 * c:]), bits(body[..., 4 * c:])), "channels beyond 4c were written"
    return [got[..., (i + 1) * c: (i + 2) * c].permute(0, 3, 1, 2).contiguous() for i in range(3)]


def check_spp(lib, case, dt, device="cpu"):
    """bit for bit wherever the reference is not a zero; where it is one, a zero of either sign: which of -0 and +0 a maximum over both returns depends on the order in
    which the window is visited (max(-0, +0) is either in IEEE 754), in the reference as much as in the kernels"""
    got = run_spp(lib, case, dt, device)
    for k, g_, r in zip((5, 9, 13), got, spp_ref(dt, case.n, case.c, case.h, case.w)):
        zero = r.float() == 0
        bad = (bits(g_) != bits(r)) & ~zero
        assert not bad.any(), f"{case.name} {dt} pool{k}: {int(bad.sum())} elements differ, first at (img, ch, y, x) = {tuple(int(v) for v in bad.nonzero()[0])}"
        assert (g_.float()[zero] == 0).all() and ((bits(g_)[zero] & 0x7fff if dt != "f32" else bits(g_)[zero] & 0x7fffffff) == 0).all(), f"{case.name} {dt} pool{k}: zeros"
    return got


# ---- 3. upsample and view copy -------------------------------------------------------------------------------------------------------------------------------------------
UP_MAPS = ((1, 1), (1, 5), (3, 2), (20, 17))
UP_SLICES = {8: ((24, 8), (40, 16)), 64: ((80, 8), (96, 24))}   # c -> ((source buffer channels, first channel), (destination buffer channels, first channel))
_INT = {"f16": torch.int16, "bf16": torch.int16, "f32": torch.int32}


def raw_patterns(dt, shape, seed):
    """arbitrary bit patterns of the element size, NaN patterns included (both kernels are typeless copies), as integers"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = (-2 ** 15, 2 ** 15) if ESZ[dt] == 2 else (-2 ** 31, 2 ** 31)
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int64).to(_INT[dt])


def _strided_case(dt, n, h, w, c, seed, device):
    (xcs, xoff), (ycs, yoff) = UP_SLICES[c]
    src = raw_patterns(dt, (n, h, w, xcs), seed)
    return src, src.to(device), xcs, xoff, ycs, yoff


def run_upsample(lib, dt, n, h, w, c, device="cpu", stream=None):
    """ymi_upsample2x from a channel slice of one buffer into a channel slice of another with a different stride -> (got bits (n, 2h, 2w, c), source bits (n, h, w, c))"""
    src, dsrc, xcs, xoff, ycs, yoff = _strided_case(dt, n, h, w, c, 11 + h * w + c, device)
    dst = Guarded((n, 2 * h, 2 * w, ycs), 2 * w * ycs, _INT[dt], device)
    esz = ESZ[dt]
    rc = lib.ymi_upsample2x(C.c_void_p(dsrc.data_ptr() + xoff * esz), xcs, n, h, w, c, C.c_void_p(dst.ptr + yoff * esz), ycs, DT_CODE[dt], stream)
    assert rc == YMI_OK, last_error(lib)
    got, before = dst.read(), dst.initial()
    assert torch.equal(got[..., :yoff], before[..., :yoff]) and torch.equal(got[..., yoff + c:], before[..., yoff + c:]), "channels outside the slice were written"
    return got[..., yoff: yoff + c], src[..., xoff: xoff + c]


def upsample_ref(src):
    """F.interpolate(scale_factor=2, mode="nearest") of the pixel index (exact in fp32), then the raw bits gathered through it"""
    n, h, w, c = src.shape
    idx = F.interpolate(torch.arange(h * w, dtype=torch.float32).view(1, 1, h, w), scale_factor=2, mode="nearest").long().view(-1)
    return src.reshape(n, h * w, c)[:, idx].view(n, 2 * h, 2 * w, c)


def run_copy(lib, dt, n, h, w, c, device="cpu", stream=None):
    """ymi_copy_view between two channel slices of different strides -> (got bits (n, h, w, c), source bits)"""
    src, dsrc, xcs, xoff, ycs, yoff = _strided_case(dt, n, h, w, c, 23 + h * w + c, device)
    dst = Guarded((n, h, w, ycs), w * ycs, _INT[dt], device)
    esz = ESZ[dt]
    rc = lib.ymi_copy_view(C.c_void_p(dsrc.data_ptr() + xoff * esz), xcs, n * h * w, c, C.c_void_p(dst.ptr + yoff * esz), ycs, DT_CODE[dt], stream)
    assert rc == YMI_OK, last_error(lib)
    got, before = dst.read(), dst.initial()
    assert torch.equal(got[..., :yoff], before[..., :yoff]) and torch.equal(got[..., yoff + c:], before[..., yoff + c:]), "channels outside the slice were written"
    return got[..., yoff: yoff + c], src[..., xoff: xoff + c]


def check_upsample_and_copy(lib, dt, h, w, device="cpu"):
    for n in (1, 3):
        for c in (8, 64):
            got, src = run_upsample(lib, dt, n, h, w, c, device)
            assert torch.equal(got, upsample_ref(src)), f"upsample {dt} n={n} {h}x{w} c={c}"
            got, src = run_copy(lib, dt, n, h, w, c, device)
            assert torch.equal(got, src), f"copy {dt} n={n} {h}x{w} c={c}"


# ---- 4. layout conversion -----------------------------------------------------------------------------------------------------------------------------------------------
LAYOUT_PAIRS = (("f32", "f16"), ("f32", "bf16"), ("f32", "f32"), ("f16", "f16"), ("f16", "f32"), ("bf16", "bf16"), ("bf16", "f32"))   # YMI_DISPATCH_IO
LAYOUT_REFUSED = (("f16", "bf16"), ("bf16", "f16"))
LAYOUT_MAPS = ((7, 9), (1, 1))
LAYOUT_BUF = (24, 8)                                 # a 24-channel NHWC buffer, the slice starts at channel 8
_SPECIALS = (1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 70000.0,   # fp16 ties of both parities, bf16 ties, overflow
             -70000.0, 65520.0, 65519.996, 3.4e38, -3.4e38, 3.39e38, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 1.0001 * 2.0 ** -25, 3e-6, 6e-8,   # fp16 subnormal results
             1e-39, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -133, -0.0, 0.0, 2.0 ** -149, -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -12, 1 + 2.0 ** -9)       # bf16 subnormal results, -0


def layout_values(in_dt, shape, seed):
    """fp32: normal values with `_SPECIALS` (ties, overflow to infinity, subnormal results, -0) at the front, rotated by the seed so that a 1 x 1 map sees other ones per
    case; 16-bit: every kind of finite pattern and the infinities (no NaN: a conversion may quiet one)"""
    g = torch.Generator().manual_seed(seed)
    numel = int(np.prod(shape))
    if in_dt == "f32":
        x = torch.randn(numel, generator=g) * 3.0
        sp = torch.tensor(_SPECIALS, dtype=torch.float64).roll(-6 * (seed % 5)).to(torch.float32)[:numel]
        x[: sp.numel()] = sp
        return x.view(shape)
    b = torch.randint(-2 ** 15, 2 ** 15, (numel,), generator=g, dtype=torch.int64).to(torch.int16)
    exp, man = (0x7c00, 0x03ff) if in_dt == "f16" else (0x7f80, 0x007f)
    nan = ((b & exp) == exp) & ((b & man) != 0)
    b = torch.where(nan, b & ~torch.tensor(man, dtype=torch.int16), b)
    x = b.view(TORCH_DT[in_dt])
    assert not torch.isnan(x.float()).any()
    return x.view(shape)


def run_to_nhwc(lib, x, in_dt, out_dt, c_pad, device="cpu", stream=None):
    """ymi_nchw_to_nhwc of x (n, c, h, w) into the slice [8, 8 + c_pad) of a poisoned 24-channel buffer -> the whole buffer (n, h, w, 24) in the output type"""
    n, c, h, w = x.shape
    ycs, yoff = LAYOUT_BUF
    dst = Guarded((n, h, w, ycs), w * ycs, TORCH_DT[out_dt], device)
    dx = (x.contiguous() if x.numel() else torch.zeros(16, dtype=x.dtype)).to(device)   # an empty tensor has no address: n == 0 still gets a valid pointer
    rc = lib.ymi_nchw_to_nhwc(C.c_void_p(dx.data_ptr()), n, c, h, w, DT_CODE[in_dt], C.c_void_p(dst.ptr + yoff * ESZ[out_dt]), ycs, c_pad, DT_CODE[out_dt], stream)
    return rc, dst.read(), dst.initial()


def run_to_nchw(lib, buf, c, in_dt, out_dt, device="cpu", stream=None):
    """ymi_nhwc_to_nchw of the slice [8, 8 + c) of a 24-channel buffer (n, h, w, 24) -> dense (n, c, h, w) between guard bands"""
    n, h, w, xcs = buf.shape
    dst = Guarded((n, c, h, w), h * w, TORCH_DT[out_dt], device)
    dx = (buf.contiguous() if buf.numel() else torch.zeros(64, dtype=buf.dtype)).to(device)
    rc = lib.ymi_nhwc_to_nchw(C.c_void_p(dx.data_ptr() + LAYOUT_BUF[1] * ESZ[in_dt]), xcs, n, c, h, w, DT_CODE[in_dt], C.c_void_p(dst.ptr), DT_CODE[out_dt], stream)
    return rc, dst.read(), dst.initial()


def check_layout(lib, in_dt, out_dt, h, w, device="cpu", n=2):
    ycs, off = LAYOUT_BUF
    tdt = TORCH_DT[out_dt]
    for c, c_pad in ((3, 4), (3, 8)):
        x = layout_values(in_dt, (n, c, h, w), seed=c_pad + h)
        rc, got, before = run_to_nhwc(lib, x, in_dt, out_dt, c_pad, device)
        assert rc == YMI_OK, last_error(lib)
        want = x.permute(0, 2, 3, 1).to(tdt)
        assert torch.equal(bits(got[..., off: off + c]), bits(want)), f"nchw -> nhwc {in_dt} -> {out_dt} c_pad {c_pad} {h}x{w}"
        assert (bits(got[..., off + c: off + c_pad]) == 0).all(), "pad channels must be +0"
        assert torch.equal(bits(got[..., :off]), bits(before[..., :off])) and torch.equal(bits(got[..., off + c_pad:]), bits(before[..., off + c_pad:])), "outside the slice"
    for c in (3, 16):
        buf = layout_values(in_dt, (n, h, w, ycs), seed=40 + c + w)
        rc, got, _ = run_to_nchw(lib, buf, c, in_dt, out_dt, device)
        assert rc == YMI_OK, last_error(lib)
        assert torch.equal(bits(got), bits(buf[..., off: off + c].permute(0, 3, 1, 2).to(tdt))), f"nhwc -> nchw {in_dt} -> {out_dt} c {c} {h}x{w}"


def check_layout_edges(lib, device="cpu"):
    """n == 0 returns YMI_OK and writes nothing; the unsupported pairs return YMI_EINVAL with a message and write nothing"""
    x = layout_values("f32", (1, 3, 2, 2), seed=1)
    rc, got, before = run_to_nhwc(lib, x[:0], "f32", "f16", 4, device)
    assert rc == YMI_OK and torch.equal(bits(got), bits(before))
    rc, got, before = run_to_nchw(lib, layout_values("f16", (1, 2, 2, 24), seed=2)[:0], 3, "f16", "f32", device)
    assert rc == YMI_OK and torch.equal(bits(got), bits(before))
    for i, o in LAYOUT_REFUSED:
        rc, got, before = run_to_nhwc(lib, layout_values(i, (1, 3, 2, 2), seed=3), i, o, 4, device)
        assert rc == YMI_EINVAL and "unsupported dtype pair" in last_error(lib) and torch.equal(bits(got), bits(before)), (i, o, rc, last_error(lib))
        rc, got, before = run_to_nchw(lib, layout_values(i, (1, 2, 2, 24), seed=4), 3, i, o, device)
        assert rc == YMI_EINVAL and "unsupported dtype pair" in last_error(lib) and torch.equal(bits(got), bits(before)), (i, o, rc, last_error(lib))
