"""Kernel LOGIC on the CPU: selected HIP kernels compiled unchanged for the host on a lane-accurate runtime (tests/hipsim/hipsim.h:
every lane a fiber, MFMA / permlane32_swap / readfirstlane / barriers / LDS-DMA restated) and driven through ctypes.

Why it exists: round 2 ended with kernels written after the GPU minutes were spent (csrc/c3_fused32.hip, the row-transposed stores
of csrc/conv1x1_stream.hip had only a partial GPU suite behind them).  This suite executes their real source -- every address,
lane mapping, barrier and store -- and compares
  * the fused one-Bottleneck C3 launch with the THREE SEPARATE LAUNCHES it replaces (streaming 1x1 with the chained 1x1, the
    resident-weights 3x3 with the shortcut, the streaming 1x1 over the concat), bit for bit, and with torch fp32;
  * the streaming 1x1 kernel (row-transposed stores, channel split, chained 1x1, residual, ragged pixel counts) with torch fp32.
The simulator is test infrastructure: the product never links it, and nothing here replaces the `-m gpu` parity tests (hardware
exp2 / rcp, timing, the real MFMA adder tree are not modelled).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _head_cases
import _post_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "hipsim")


def _clangxx():
    for c in (os.environ.get("HIPSIM_CXX"), "/opt/rocm/lib/llvm/bin/clang++", shutil.which("amdclang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def sim():
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no host clang++ (ext_vector_type / _Float16 / __bf16 sources need clang)")
    out_dir = os.path.join(SIM_DIR, "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libhipsim_kernels.so")
    units = ["sim_kernels", "sim_kernels_gemm", "sim_kernels_v2", "sim_kernels_pre", "sim_kernels_post", "sim_kernels_stem", "sim_kernels_f32", "sim_kernels_f32p", "sim_kernels_c3t"]   # translation units, compiled in parallel (-O0: ~10 s; the optimiser would take two minutes and save one)
    csrc = os.path.join(ROOT, "yolort_amd", "csrc")
    srcs = [os.path.join(SIM_DIR, f) for f in ("hipsim.h", "hipsim.cpp", "sim_fill.h")] + [os.path.join(SIM_DIR, u + ".cpp") for u in units] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hpp", ".hip")) and not f.startswith(("conv_inst", "head_inst"))] + \
           [os.path.join(ROOT, "include", "yolort_amd.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        flags = ["-std=c++17", os.environ.get("HIPSIM_OPT", "-O0"), "-fPIC", "-ffp-contract=off", "-I", SIM_DIR, "-I", os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-psabi", "-Wno-pass-failed"]
        # postprocess.hip declares STATIC __shared__ arrays: its unit is built with -D__shared__=static from a copy of the source in
        # which `extern __shared__` lost the keyword (the only textual change any kernel source sees here)
        with open(os.path.join(csrc, "postprocess.hip")) as f:
            text = f.read()
        with open(os.path.join(out_dir, "postprocess.sim.hip"), "w") as f:
            f.write(text.replace("extern __shared__", "extern"))
        extra = {"sim_kernels_post": ["-D__shared__=static", "-I", out_dir, "-I", csrc], "sim_kernels_stem": ["-D__shared__=static"], "sim_kernels_f32": ["-D__shared__=static"]}
        procs = [subprocess.Popen([cxx, *flags, *extra.get(u, []), "-c", os.path.join(SIM_DIR, u + ".cpp"), "-o", os.path.join(out_dir, u + ".o")]) for u in units]
        assert all(p.wait() == 0 for p in procs), "the simulator build failed"
        subprocess.run([cxx, "-shared", "-o", so] + [os.path.join(out_dir, u + ".o") for u in units], check=True)
    lib = C.CDLL(so)
    from yolort_amd._lib import C3Desc, ConvDesc
    lib.sim_c3_fused.argtypes, lib.sim_c3_fused.restype = [C.POINTER(C3Desc)], C.c_int
    lib.sim_conv2d.argtypes, lib.sim_conv2d.restype = [C.POINTER(ConvDesc)], C.c_int
    lib.sim_c3_tile.argtypes, lib.sim_c3_tile.restype = [C.POINTER(C3Desc)], C.c_int
    lib.ymi_c3_blob_bytes.argtypes, lib.ymi_c3_blob_bytes.restype = [C.POINTER(C3Desc)], C.c_int64
    lib.ymi_c3_pack.argtypes, lib.ymi_c3_pack.restype = [C.POINTER(C3Desc), C.c_void_p, C.c_void_p], C.c_int
    lib.ymi_c3_tile_supported.argtypes, lib.ymi_c3_tile_supported.restype = [C.POINTER(C3Desc)], C.c_int
    lib.sim_conv_f32_pick_tile.argtypes, lib.sim_conv_f32_pick_tile.restype = [C.c_int, C.c_int], C.c_int
    lib.sim_last_error.restype = C.c_char_p
    lib.sim_max_lds.restype = C.c_int
    lib.ymi_letterbox.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]
    lib.ymi_nms_ws_bytes.argtypes, lib.ymi_nms_ws_bytes.restype = [C.c_int], C.c_int64
    lib.sim_conv_stem_planar.argtypes, lib.sim_conv_stem_planar.restype = [C.POINTER(ConvDesc), C.POINTER(C.c_void_p), C.c_int], C.c_int
    lib.sim_stem_body1_planar.argtypes, lib.sim_stem_body1_planar.restype = [C.POINTER(ConvDesc), C.POINTER(ConvDesc), C.POINTER(C.c_void_p), C.c_int], C.c_int
    lib.sim_stem_body1.argtypes, lib.sim_stem_body1.restype = [C.POINTER(ConvDesc), C.POINTER(ConvDesc)], C.c_int
    from yolort_amd._lib import PostDesc
    lib.ymi_postprocess_ws_bytes.argtypes, lib.ymi_postprocess_ws_bytes.restype = [C.c_int, C.c_int, C.c_int], C.c_int64
    lib.ymi_postprocess.argtypes, lib.ymi_postprocess.restype = [C.POINTER(PostDesc), C.c_void_p], C.c_int
    lib.ymi_post_begin.argtypes, lib.ymi_post_finish.argtypes = [C.POINTER(PostDesc), C.c_void_p], [C.POINTER(PostDesc), C.c_void_p]
    lib.sim_conv_head_decode_group.argtypes, lib.sim_conv_head_decode_group.restype = [C.POINTER(ConvDesc), C.c_int, C.POINTER(PostDesc)], C.c_int
    lib.ymi_batched_nms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.ymi_copy_view.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.ymi_act.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.ymi_nchw_to_nhwc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.ymi_nhwc_to_nchw.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.ymi_spp_pool.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.ymi_upsample2x.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def _check(lib, rc):
    assert rc == 0, lib.sim_last_error().decode()


class Buf:
    """NHWC host buffer with the 256-byte zero tail plan buffers carry (source of out-of-image operand chunks)"""

    def __init__(self, n, h, w, c, dtype, fill=None):
        self.n, self.h, self.w, self.c, self.cs, self.off = n, h, w, c, c, 0
        numel = (n * h * w * c + 7) // 8 * 8
        self.t = torch.zeros(numel + 128, dtype=dtype)
        self.numel = numel
        if fill is not None:
            self.t[: n * h * w * c] = fill.reshape(-1).to(dtype)

    def view(self):
        return torch.as_strided(self.t, (self.n, self.h, self.w, self.c), (self.h * self.w * self.cs, self.w * self.cs, self.cs, 1), self.off)

    def slice_c(self, c0, c):
        v = Buf.__new__(Buf)
        v.__dict__.update(self.__dict__)
        v.off, v.c = self.off + c0, c
        return v

    @property
    def ptr(self):
        return self.t.data_ptr() + 2 * self.off

    @property
    def zeros(self):
        return self.t.data_ptr() + 2 * self.numel


def _conv_desc(x, pc, y, tile, k=1, pad=0, res=None, y2=None, split=0, chain=None, stride=1):
    from yolort_amd._lib import ACT_SILU, ConvDesc, dtype_code
    d = ConvDesc()
    d.x, d.w, d.bias, d.y = x.ptr, pc.w.data_ptr(), pc.bias.data_ptr(), y.ptr
    d.res = None if res is None else res.ptr
    d.n, d.h, d.w_in, d.cin, d.x_cstride = x.n, x.h, x.w, pc.cin, x.cs
    d.ho, d.wo, d.cout, d.cout_pad, d.y_cstride = y.h, y.w, pc.cout, pc.cout_pad, y.cs
    d.res_cstride = 0 if res is None else res.cs
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.k_pad = k, k, stride, stride, pad, pad, pc.k_pad
    d.act, d.dtype, d.out_dtype, d.tile = ACT_SILU, dtype_code(pc.dtype), dtype_code(pc.dtype), tile
    if y2 is not None:
        d.y2, d.y2_cstride, d.cout_split = y2.ptr, y2.cs, split
    if chain is not None:
        pc2, tv = chain
        d.chain_w, d.chain_bias, d.chain_y, d.chain_cout, d.chain_y_cstride = pc2.w.data_ptr(), pc2.bias.data_ptr(), tv.ptr, pc2.cout, tv.cs
    d.zeros = x.zeros
    return d


def _make_c3(seed):
    from yolort_amd.v5.models.common import C3
    torch.manual_seed(seed)
    m = C3(64, 64, n=1).eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.6, 1.4)
                mod.bias.normal_(0, 0.2)
                mod.running_mean.normal_(0, 0.3)
                mod.running_var.uniform_(0.5, 1.5)
    return m


def _torch_conv(c, t, dtype, res=None):
    bn = c.bn
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    w = (c.conv.weight * scale.view(-1, 1, 1, 1)).to(dtype).float()
    y = F.silu(F.conv2d(t, w, bn.bias - bn.running_mean * scale, c.conv.stride, c.conv.padding))
    if res is not None:
        y = y + res
    return y.to(dtype).float()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
# (5, 112, 128): 280 tiles on a grid of 256 persistent blocks -- the second trip through the tile loop (patch reuse behind the barriers)
@pytest.mark.parametrize("shape", [(1, 16, 16), (2, 21, 37), (1, 5, 3), (1, 33, 16), (5, 112, 128)])
def test_fused_c3_equals_the_three_launches_and_torch(sim, dtype, shape):
    from yolort_amd._lib import C3Desc, dtype_code
    n, h, w = shape
    if n * h * w > 20000 and dtype == torch.bfloat16:
        pytest.skip("the large case runs once (fp16)")
    m = _make_c3(seed=h * 7 + w)
    cpu = torch.device("cpu")
    x = torch.randn(n, 64, h, w, generator=torch.Generator().manual_seed(n + h)).to(dtype).float()
    xb = Buf(n, h, w, 64, dtype, fill=x.permute(0, 2, 3, 1))
    pc12 = m.packed_pair(dtype, cpu, 64)
    b0 = m.m[0]
    pcm1, pcm2, pc3 = b0.cv1.packed(dtype, cpu, 32), b0.cv2.packed(dtype, cpu, 32), m.cv3.packed(dtype, cpu, 64)

    # ---- the three launches C3.emit records by default (tiles of the pinned table for this layer) ----
    y1, t0, cat, out_sep = Buf(n, h, w, 32, dtype), Buf(n, h, w, 32, dtype), Buf(n, h, w, 64, dtype), Buf(n, h, w, 64, dtype)
    _check(sim, sim.sim_conv2d(C.byref(_conv_desc(xb, pc12, y1, 121, y2=cat.slice_c(32, 32), split=32, chain=(pcm1, t0)))))
    _check(sim, sim.sim_conv2d(C.byref(_conv_desc(t0, pcm2, cat.slice_c(0, 32), 131, k=3, pad=1, res=y1))))
    _check(sim, sim.sim_conv2d(C.byref(_conv_desc(cat, pc3, out_sep, 122))))

    # ---- the fused launch ----
    out_f = Buf(n, h, w, 64, dtype)
    d = C3Desc()
    d.x, d.y = xb.ptr, out_f.ptr
    d.w12, d.b12, d.wm1, d.bm1 = pc12.w.data_ptr(), pc12.bias.data_ptr(), pcm1.w.data_ptr(), pcm1.bias.data_ptr()
    d.wm2, d.bm2, d.w3, d.b3 = pcm2.w.data_ptr(), pcm2.bias.data_ptr(), pc3.w.data_ptr(), pc3.bias.data_ptr()
    d.n, d.h, d.w, d.x_cstride, d.y_cstride, d.dtype = n, h, w, 64, 64, dtype_code(dtype)
    d.c_in, d.c_hidden, d.c_out, d.n_bottlenecks, d.shortcut = 64, 32, 64, 1, 1
    d.k12_pad, d.km1_pad, d.km2_pad, d.k3_pad = pc12.k_pad, pcm1.k_pad, pcm2.k_pad, pc3.k_pad
    _check(sim, sim.sim_c3_fused(C.byref(d)))
    assert sim.sim_max_lds() <= 64 * 1024   # no launch of this test may need the > 64 KiB opt-in

    a, b = out_sep.view(), out_f.view()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"fused vs separate launches: max difference {(a.float() - b.float()).abs().max().item()}"
    with torch.no_grad():
        x1, x2 = _torch_conv(m.cv1, x, dtype), _torch_conv(m.cv2, x, dtype)
        v = _torch_conv(b0.cv2, _torch_conv(b0.cv1, x1, dtype), dtype, res=x1)
        ref = _torch_conv(m.cv3, torch.cat([v, x2], 1), dtype).permute(0, 2, 3, 1)
    tol = 4e-3 if dtype == torch.float16 else 3.2e-2
    err = (b.float() - ref).abs().max().item()
    assert err <= tol * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("tile", [121, 122, 124])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_streaming_1x1_kernel_logic(sim, dtype, tile):
    """conv1x1_stream.hip as the plan uses it: whole cout blocks (row-transposed stores), a ragged last pixel group, channel-slice
    output views, residual, and -- tile 121 / 122 -- the channel split with the chained 1x1"""
    from yolort_amd import engine
    cpu = torch.device("cpu")
    tnw = tile - 120
    g = torch.Generator().manual_seed(tile)
    for cin, cout, n, h, w, residual in [(64, 32 * tnw, 2, 9, 7, True), (32, 64 * tnw, 1, 13, 5, False), (128, 32 * tnw, 1, 6, 11, False)]:
        x = torch.randn(n, cin, h, w, generator=g).to(dtype).float()
        wt = (torch.randn(cout, cin, 1, 1, generator=g) / np.sqrt(cin)).to(dtype).float()
        bias = torch.randn(cout, generator=g) * 0.1
        ref = F.silu(F.conv2d(x, wt, bias))
        pc = engine.PackedConv(wt, bias, None, dtype, cpu)
        xb = Buf(n, h, w, cin, dtype, fill=x.permute(0, 2, 3, 1))
        wide = Buf(n, h, w, cout + 64, dtype)           # the output is a channel slice of a wider buffer
        yv = wide.slice_c(32, cout)
        rb = None
        if residual:
            r = torch.randn(n, cout, h, w, generator=g).to(dtype).float()
            ref = ref + r
            rb = Buf(n, h, w, cout, dtype, fill=r.permute(0, 2, 3, 1))
        _check(sim, sim.sim_conv2d(C.byref(_conv_desc(xb, pc, yv, tile, res=rb))))
        got = yv.view().float().permute(0, 3, 1, 2)
        tol = 2e-3 if dtype == torch.float16 else 1.6e-2
        assert (got - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())
        w_all = wide.view().float()
        assert w_all[..., :32].abs().max().item() == 0 and w_all[..., 32 + cout:].abs().max().item() == 0   # nothing outside the slice
    if tnw <= 2:   # channel split + chained 1x1 (cv1 | cv2 of a C3 with the first Bottleneck's 1x1 riding along)
        k1 = 32 * tnw
        x = torch.randn(2, 64, 7, 9, generator=g).to(dtype).float()
        wt = (torch.randn(2 * k1, 64, 1, 1, generator=g) / 8).to(dtype).float()
        bias = torch.randn(2 * k1, generator=g) * 0.1
        w2 = (torch.randn(k1, k1, 1, 1, generator=g) / np.sqrt(k1)).to(dtype).float()
        b2 = torch.randn(k1, generator=g) * 0.1
        full = F.silu(F.conv2d(x, wt, bias)).to(dtype).float()
        chained = F.silu(F.conv2d(full[:, :k1], w2, b2))
        pc, pc2 = engine.PackedConv(wt, bias, None, dtype, cpu), engine.PackedConv(w2, b2, None, dtype, cpu)
        xb = Buf(2, 7, 9, 64, dtype, fill=x.permute(0, 2, 3, 1))
        y1, cat, tb = Buf(2, 7, 9, k1, dtype), Buf(2, 7, 9, 2 * k1, dtype), Buf(2, 7, 9, k1, dtype)
        _check(sim, sim.sim_conv2d(C.byref(_conv_desc(xb, pc, y1, tile, y2=cat.slice_c(k1, k1), split=k1, chain=(pc2, tb)))))
        tol = 2e-3 if dtype == torch.float16 else 1.6e-2
        assert torch.equal(y1.view().float(), full[:, :k1].permute(0, 2, 3, 1)) or (y1.view().float() - full[:, :k1].permute(0, 2, 3, 1)).abs().max().item() <= tol * full.abs().max().item()
        assert (cat.view().float()[..., k1:] - full[:, k1:].permute(0, 2, 3, 1)).abs().max().item() <= tol * max(1.0, full.abs().max().item())
        assert cat.view().float()[..., :k1].abs().max().item() == 0   # the first half of the concat belongs to the Bottleneck
        assert (tb.view().float() - chained.permute(0, 2, 3, 1)).abs().max().item() <= 2 * tol * max(1.0, chained.abs().max().item())


def _run_conv(sim, dtype, tile, n, cin, cout, h, w, k, s, residual=False, seed=0):
    """one convolution through the simulator against torch fp32 on the same rounded operands (bound of tests/test_ops_gpu.py)"""
    from yolort_amd import engine
    g = torch.Generator().manual_seed(seed)
    p = k // 2
    x = torch.randn(n, cin, h, w, generator=g).to(dtype).float()
    wt = (torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)).to(dtype).float()
    bias = torch.randn(cout, generator=g) * 0.1
    ref = F.silu(F.conv2d(x, wt, bias, s, p))
    ho, wo = ref.shape[2], ref.shape[3]
    pc = engine.PackedConv(wt, bias, None, dtype, torch.device("cpu"))
    xb = Buf(n, h, w, cin, dtype, fill=x.permute(0, 2, 3, 1))
    wide = Buf(n, ho, wo, cout + 32, dtype)
    yv = wide.slice_c(16, cout)
    rb = None
    if residual:
        r = torch.randn(n, cout, ho, wo, generator=g).to(dtype).float()
        ref = ref + r
        rb = Buf(n, ho, wo, cout, dtype, fill=r.permute(0, 2, 3, 1))
    d = _conv_desc(xb, pc, yv, tile, k=k, pad=p, res=rb, stride=s)
    if k > 1:
        kt = pc.ktab(w, xb.cs)   # the im2col table of the general-tap kernels (cin % 32 != 0); the uniform-tap kernels ignore it
        d.ktab = kt.data_ptr()
    _check(sim, sim.sim_conv2d(C.byref(d)))
    got = yv.view().float().permute(0, 3, 1, 2)
    tol = 2e-3 if dtype == torch.float16 else 1.6e-2
    assert (got - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item()), (tile, cin, cout, k, s)
    w_all = wide.view().float()
    assert w_all[..., :16].abs().max().item() == 0 and w_all[..., 16 + cout:].abs().max().item() == 0
    return yv.view().clone()


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cout", [32, 64])
def test_resident_weights_3x3_kernel_logic(sim, stride, cout):
    """conv3x3_c32.hip (tile 131): both strides (parity-split patch columns), ragged maps, the shortcut"""
    for dtype, (n, h, w) in [(torch.float16, (2, 13, 21)), (torch.bfloat16, (1, 8, 16)), (torch.float16, (1, 5, 7))]:
        _run_conv(sim, dtype, 131, n, 32, cout, h, w, 3, stride, residual=(stride == 1 and cout == 32), seed=cout + stride)


@pytest.mark.parametrize("tile,cout", [(91, 128), (92, 64), (93, 64), (94, 32), (95, 128)])
def test_halo8_3x3_kernel_logic(sim, tile, cout):
    """conv_halo8.hip: every wave layout; one and two 32-channel chunks (single / double patch buffer), ragged maps, the shortcut"""
    _run_conv(sim, torch.float16, tile, 2, 64, cout, 9, 12, 3, 1, residual=True, seed=tile)
    _run_conv(sim, torch.bfloat16, tile, 1, 32, cout, 20, 20, 3, 1, seed=tile + 1)


def test_igemm8_192_cout_blocks_equal_the_128_wide_tile(sim):
    """round 4: conv_igemm8_kernel<.., 192, 4, ..> (tile 120: 4 x 2 waves of 64 pixels x 96 couts; yolov5m's 192-cout layers): against torch and BIT-IDENTICAL to tile 111,
    strided 3x3 / 1x1 / 3x3 with a shortcut, one and two cout blocks, ragged maps, both 16-bit types"""
    for dtype, (n, cin, cout, h, w, k, s_, res) in [(torch.float16, (2, 96, 192, 13, 11, 3, 2, False)), (torch.bfloat16, (1, 64, 384, 9, 10, 1, 1, True)), (torch.float16, (1, 32, 192, 8, 7, 3, 1, True))]:
        a = _run_conv(sim, dtype, 111, n, cin, cout, h, w, k, s_, residual=res, seed=120 + cin)
        b = _run_conv(sim, dtype, 120, n, cin, cout, h, w, k, s_, residual=res, seed=120 + cin)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (dtype, cin, cout, k, s_)


def test_halo8_96_cout_blocks_equal_the_128_wide_tile(sim):
    """round 4: conv_halo8_kernel<.., 96, 8> (tile 96: 8 x 1 waves of 32 pixels x 96 couts -- yolov5m's 96 -> 96 and 192 -> 192 3x3 layers without the idle quarter of a 128-wide
    block): against torch and BIT-IDENTICAL to tile 91 (same K order), one and two cout blocks, with a shortcut, ragged maps, both 16-bit types, two and three channel chunks"""
    for dtype, (n, cin, cout, h, w, res) in [(torch.float16, (2, 96, 96, 9, 12, True)), (torch.bfloat16, (1, 64, 192, 20, 20, False)), (torch.float16, (1, 96, 192, 7, 5, True))]:
        a = _run_conv(sim, dtype, 91, n, cin, cout, h, w, 3, 1, residual=res, seed=96 + cin)
        b = _run_conv(sim, dtype, 96, n, cin, cout, h, w, 3, 1, residual=res, seed=96 + cin)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (dtype, cin, cout)


@pytest.mark.parametrize("tile,c_,residual", [(93, 64, True), (93, 64, False), (95, 128, True), (94, 32, True)])
def test_halo8_with_a_chained_1x1_equals_the_two_launches(sim, tile, c_, residual):
    """conv_halo8.hip, 8 x 1 wave forms, with the NEXT Bottleneck's 1x1 riding in the epilogue (round 3: m.j.cv2 + m.(j+1).cv1 as one launch,
    reference common.py:115-116 twice): the 3x3's own output and the chained 1x1's output equal the two separate launches bit for bit"""
    from yolort_amd import engine
    dtype, cpu = torch.float16, torch.device("cpu")
    g = torch.Generator().manual_seed(tile + c_)
    n, h, w = 2, 11, 13
    x = torch.randn(n, c_, h, w, generator=g).to(dtype).float()
    w3 = (torch.randn(c_, c_, 3, 3, generator=g) / np.sqrt(9 * c_)).to(dtype).float()
    b3 = torch.randn(c_, generator=g) * 0.1
    w1 = (torch.randn(c_, c_, 1, 1, generator=g) / np.sqrt(c_)).to(dtype).float()
    b1 = torch.randn(c_, generator=g) * 0.1
    pc3, pc1 = engine.PackedConv(w3, b3, None, dtype, cpu), engine.PackedConv(w1, b1, None, dtype, cpu)
    xb = Buf(n, h, w, c_, dtype, fill=x.permute(0, 2, 3, 1))
    rb = None
    if residual:
        rb = Buf(n, h, w, c_, dtype, fill=torch.randn(n, h, w, c_, generator=g))
    kt = pc3.ktab(w, c_)

    def d3(y, chain=None):
        d = _conv_desc(xb, pc3, y, tile, k=3, pad=1, res=rb, chain=chain)
        d.ktab = kt.data_ptr()
        return d

    y_sep, t_sep = Buf(n, h, w, c_, dtype), Buf(n, h, w, c_, dtype)
    _check(sim, sim.sim_conv2d(C.byref(d3(y_sep))))
    _check(sim, sim.sim_conv2d(C.byref(_conv_desc(y_sep, pc1, t_sep, 27 if c_ <= 64 else 21))))
    y_ch, t_ch = Buf(n, h, w, c_, dtype), Buf(n, h, w, c_, dtype)
    _check(sim, sim.sim_conv2d(C.byref(d3(y_ch, chain=(pc1, t_ch)))))
    assert torch.equal(y_ch.view().view(torch.int16), y_sep.view().view(torch.int16))
    assert torch.equal(t_ch.view().view(torch.int16), t_sep.view().view(torch.int16)), (t_ch.view().float() - t_sep.view().float()).abs().max().item()
    ref = F.silu(F.conv2d(x, w3, b3, 1, 1))
    if residual:
        ref = ref + rb.view().float().permute(0, 3, 1, 2)
    ref1 = F.silu(F.conv2d(ref.to(dtype).float(), w1, b1)).permute(0, 2, 3, 1)
    assert (t_ch.view().float() - ref1).abs().max().item() <= 4e-3 * max(1.0, ref1.abs().max().item())


@pytest.mark.parametrize("cin,cout,xcs", [(64, 64, 64), (64, 48, 64), (48, 48, 48), (64, 32, 96), (48, 64, 64)])
def test_resident_weights_3x3_c64_kernel_logic(sim, cin, cout, xcs, monkeypatch):
    """conv3x3_res.hip (tile 132): 48 / 64 input channels, resident weights, persistent blocks with the next tile's patch in flight -- against
    torch, and BIT-IDENTICAL to the 8-wave implicit GEMM (tiles 113 / 114: the same K order -- tap-major, channel-minor; the halo kernel it replaces
    walks 32-channel chunks outermost and rounds differently in the last bit); maps that are ragged against the 16 x 16 tiles, several
    tiles per block (the double-buffered patch), the shortcut, a channel-slice input view (pixel stride > cin)"""
    from yolort_amd import engine
    cpu = torch.device("cpu")
    monkeypatch.setenv("YOLORT_AMD_RES3X3_BLOCKS", "3")   # 12 / 1 / 4 tiles on 3 blocks: the persistent loop, both patch buffers, the deferred stores
    for dtype, (n, h, w), residual in [(torch.float16, (2, 21, 37), True), (torch.bfloat16, (1, 16, 16), False), (torch.float16, (1, 5, 50), False)]:
        g = torch.Generator().manual_seed(cin + cout + h)
        x = torch.randn(n, cin, h, w, generator=g).to(dtype).float()
        wt = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).to(dtype).float()
        bias = torch.randn(cout, generator=g) * 0.1
        pc = engine.PackedConv(wt, bias, None, dtype, cpu)
        xw = Buf(n, h, w, xcs, dtype)
        xw.view()[..., :cin] = x.permute(0, 2, 3, 1).to(dtype)
        if xcs > cin:
            xw.view()[..., cin:] = 7.0     # the neighbouring channels of the slice must not leak in
        xb = xw.slice_c(0, cin)
        rb = Buf(n, h, w, cout, dtype, fill=torch.randn(n, h, w, cout, generator=g)) if residual else None
        ref = F.silu(F.conv2d(x, wt, bias, 1, 1))
        if residual:
            ref = ref + rb.view().float().permute(0, 3, 1, 2)
        outs = []
        for tile in ((132, 113 if cout > 32 else 114) if cin % 32 == 0 else (132,)) + ((133,) if cout == 64 else ()):
            wide = Buf(n, h, w, cout + 32, dtype)
            yv = wide.slice_c(16, cout)
            d = _conv_desc(xb, pc, yv, tile, k=3, pad=1, res=rb)
            d.ktab = pc.ktab(w, xcs).data_ptr()
            _check(sim, sim.sim_conv2d(C.byref(d)))
            got = yv.view().float().permute(0, 3, 1, 2)
            tol = 2e-3 if dtype == torch.float16 else 1.6e-2
            assert (got - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item()), (tile, cin, cout)
            w_all = wide.view().float()
            assert w_all[..., :16].abs().max().item() == 0 and w_all[..., 16 + cout:].abs().max().item() == 0
            outs.append(yv.view().clone())
        for o in outs[1:]:   # the implicit GEMM (cin % 32 == 0) and the register-weights variant (tile 133, cout = 64)
            assert torch.equal(outs[0].view(torch.int16), o.view(torch.int16)), "tile 132 differs from the implicit GEMM / tile 133"


def test_register_weights_3x3_stride2_kernel_logic(sim, monkeypatch):
    """conv3x3_rw2.hip (tile 134, round 4): 64 -> 128 at stride 2, weights in registers, parity-split double-buffered patch -- against torch, and
    BIT-IDENTICAL to the 8-wave implicit GEMM (tiles 111 / 112: the same K order); maps ragged against the 8 x 8 tiles (odd and even input sizes), several
    tiles per block, a channel-slice input view and a channel-slice output view"""
    from yolort_amd import engine
    cpu = torch.device("cpu")
    cin, cout = 64, 128
    monkeypatch.setenv("YOLORT_AMD_RES3X3_BLOCKS", "3")
    for dtype, (n, h, w), xcs in [(torch.float16, (2, 35, 50), 96), (torch.bfloat16, (1, 32, 32), 64), (torch.float16, (1, 7, 66), 64)]:
        g = torch.Generator().manual_seed(134 + h)
        x = torch.randn(n, cin, h, w, generator=g).to(dtype).float()
        wt = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).to(dtype).float()
        bias = torch.randn(cout, generator=g) * 0.1
        pc = engine.PackedConv(wt, bias, None, dtype, cpu)
        xw = Buf(n, h, w, xcs, dtype)
        xw.view()[..., :cin] = x.permute(0, 2, 3, 1).to(dtype)
        if xcs > cin:
            xw.view()[..., cin:] = 7.0     # the neighbouring channels of the slice must not leak in
        xb = xw.slice_c(0, cin)
        ref = F.silu(F.conv2d(x, wt, bias, 2, 1))
        ho, wo = ref.shape[-2:]
        outs = []
        for tile in (134, 111, 112):
            wide = Buf(n, ho, wo, cout + 32, dtype)
            yv = wide.slice_c(16, cout)
            d = _conv_desc(xb, pc, yv, tile, k=3, pad=1, stride=2)
            d.ktab = pc.ktab(w, xcs).data_ptr()
            _check(sim, sim.sim_conv2d(C.byref(d)))
            got = yv.view().float().permute(0, 3, 1, 2)
            tol = 2e-3 if dtype == torch.float16 else 1.6e-2
            assert (got - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item()), (tile, h, w)
            w_all = wide.view().float()
            assert w_all[..., :16].abs().max().item() == 0 and w_all[..., 16 + cout:].abs().max().item() == 0
            outs.append(yv.view().clone())
        for o in outs[1:]:
            assert torch.equal(outs[0].view(torch.int16), o.view(torch.int16)), "tile 134 differs from the implicit GEMM"


@pytest.mark.parametrize("stride", [1, 2])
def test_row_streaming_3x3_kernel_logic(sim, stride, monkeypatch):
    """conv3x3_rs.hip (tiles 137 / 138, round 4): a block walks down a 16-column strip of the output with a ring of input rows in LDS, the images of a strip
    concatenated into one stream (zero rows between them), row groups D steps ahead -- against torch and BIT-IDENTICAL to the implicit GEMM (tiles 113 / 111); several
    images (the stream crosses image boundaries inside a block), maps ragged against the 16-column strips and the 2 / 4-row steps, heights that are / are not multiples
    of four, few blocks (long chunks: the ring wraps many times) and many blocks (chunks shorter than the lookahead), channel-slice views on both sides"""
    from yolort_amd import engine
    cpu = torch.device("cpu")
    cin, cout, tile, ref_tile = 64, (64 if stride == 1 else 128), (137 if stride == 1 else 138), (113 if stride == 1 else 111)
    for blocks, dtype, (n, h, w), xcs in [("3", torch.float16, (3, 21, 37), 96), ("64", torch.bfloat16, (2, 16, 32), 64), ("5", torch.float16, (1, 9, 50), 64), ("2", torch.float16, (4, 8, 16), 64)]:
        monkeypatch.setenv("YOLORT_AMD_RES3X3_BLOCKS", blocks)
        g = torch.Generator().manual_seed(137 + h + stride)
        x = torch.randn(n, cin, h, w, generator=g).to(dtype).float()
        wt = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).to(dtype).float()
        bias = torch.randn(cout, generator=g) * 0.1
        pc = engine.PackedConv(wt, bias, None, dtype, cpu)
        xw = Buf(n, h, w, xcs, dtype)
        xw.view()[..., :cin] = x.permute(0, 2, 3, 1).to(dtype)
        if xcs > cin:
            xw.view()[..., cin:] = 7.0
        xb = xw.slice_c(0, cin)
        ref = F.silu(F.conv2d(x, wt, bias, stride, 1))
        ho, wo = ref.shape[-2:]
        outs = []
        for t in (tile, ref_tile):
            wide = Buf(n, ho, wo, cout + 32, dtype)
            yv = wide.slice_c(16, cout)
            d = _conv_desc(xb, pc, yv, t, k=3, pad=1, stride=stride)
            d.ktab = pc.ktab(w, xcs).data_ptr()
            _check(sim, sim.sim_conv2d(C.byref(d)))
            got = yv.view().float().permute(0, 3, 1, 2)
            tol = 2e-3 if dtype == torch.float16 else 1.6e-2
            assert (got - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item()), (t, blocks, h, w)
            w_all = wide.view().float()
            assert w_all[..., :16].abs().max().item() == 0 and w_all[..., 16 + cout:].abs().max().item() == 0
            outs.append(yv.view().clone())
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "the row-streaming kernel differs from the implicit GEMM"


@pytest.mark.parametrize("cout", [128, 256])
def test_register_weights_3x3_stride2_ksplit_kernel_logic(sim, cout, monkeypatch):
    """conv3x3_rw2.hip tile 135 (round 4): 128 -> 128 / 256 at stride 2, K split over two waves whose partial sums meet in the consumed patch buffer -- against torch
    and against the 8-wave implicit GEMM (tile 111) within the fp32 summation-order noise (the split sum is another rounding order: not bit-identical by design);
    ragged maps, several tiles per block, channel-slice views on both sides, both cout halves of the 256-wide form"""
    from yolort_amd import engine
    cpu = torch.device("cpu")
    cin = 128
    monkeypatch.setenv("YOLORT_AMD_RES3X3_BLOCKS", "2")
    for dtype, (n, h, w), xcs in [(torch.float16, (2, 19, 34), 160), (torch.bfloat16, (1, 16, 16), 128)]:
        g = torch.Generator().manual_seed(135 + h + cout)
        x = torch.randn(n, cin, h, w, generator=g).to(dtype).float()
        wt = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).to(dtype).float()
        bias = torch.randn(cout, generator=g) * 0.1
        pc = engine.PackedConv(wt, bias, None, dtype, cpu)
        xw = Buf(n, h, w, xcs, dtype)
        xw.view()[..., :cin] = x.permute(0, 2, 3, 1).to(dtype)
        if xcs > cin:
            xw.view()[..., cin:] = 7.0
        xb = xw.slice_c(0, cin)
        ref = F.silu(F.conv2d(x, wt, bias, 2, 1))
        ho, wo = ref.shape[-2:]
        outs = []
        for tile in (135, 111):
            wide = Buf(n, ho, wo, cout + 32, dtype)
            yv = wide.slice_c(16, cout)
            d = _conv_desc(xb, pc, yv, tile, k=3, pad=1, stride=2)
            d.ktab = pc.ktab(w, xcs).data_ptr()
            _check(sim, sim.sim_conv2d(C.byref(d)))
            got = yv.view().float().permute(0, 3, 1, 2)
            tol = 2e-3 if dtype == torch.float16 else 1.6e-2
            assert (got - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item()), (tile, h, w)
            w_all = wide.view().float()
            assert w_all[..., :16].abs().max().item() == 0 and w_all[..., 16 + cout:].abs().max().item() == 0
            outs.append(yv.view().float())
        ulp = 2.0 ** (-10 if dtype == torch.float16 else -7)
        assert (outs[0] - outs[1]).abs().max().item() <= ulp * max(1.0, ref.abs().max().item())   # one unit in the last place of the output type at most
        assert (outs[0] != outs[1]).float().mean().item() < 0.05


def test_resident_weights_3x3_c64_with_a_chained_1x1_equals_the_two_launches(sim):
    """tile 132 with the next Bottleneck's 1x1 riding in the epilogue (a wave owns all couts of its pixels, as in conv_halo8's 8 x 1 forms)"""
    from yolort_amd import engine
    dtype, cpu, c_ = torch.float16, torch.device("cpu"), 64
    os.environ["YOLORT_AMD_RES3X3_BLOCKS"] = "5"
    g = torch.Generator().manual_seed(132)
    n, h, w = 2, 19, 23
    x = torch.randn(n, c_, h, w, generator=g).to(dtype).float()
    w3 = (torch.randn(c_, c_, 3, 3, generator=g) / np.sqrt(9 * c_)).to(dtype).float()
    b3 = torch.randn(c_, generator=g) * 0.1
    w1 = (torch.randn(c_, c_, 1, 1, generator=g) / np.sqrt(c_)).to(dtype).float()
    b1 = torch.randn(c_, generator=g) * 0.1
    pc3, pc1 = engine.PackedConv(w3, b3, None, dtype, cpu), engine.PackedConv(w1, b1, None, dtype, cpu)
    xb = Buf(n, h, w, c_, dtype, fill=x.permute(0, 2, 3, 1))
    rb = Buf(n, h, w, c_, dtype, fill=torch.randn(n, h, w, c_, generator=g))
    kt = pc3.ktab(w, c_)

    def d3(y, tile, chain=None):
        d = _conv_desc(xb, pc3, y, tile, k=3, pad=1, res=rb, chain=chain)
        d.ktab = kt.data_ptr()
        return d

    y_sep, t_sep = Buf(n, h, w, c_, dtype), Buf(n, h, w, c_, dtype)
    _check(sim, sim.sim_conv2d(C.byref(d3(y_sep, 113))))
    _check(sim, sim.sim_conv2d(C.byref(_conv_desc(y_sep, pc1, t_sep, 27))))
    y_ch, t_ch = Buf(n, h, w, c_, dtype), Buf(n, h, w, c_, dtype)
    try:
        _check(sim, sim.sim_conv2d(C.byref(d3(y_ch, 132, chain=(pc1, t_ch)))))
    finally:
        del os.environ["YOLORT_AMD_RES3X3_BLOCKS"]
    assert torch.equal(y_ch.view().view(torch.int16), y_sep.view().view(torch.int16))
    assert torch.equal(t_ch.view().view(torch.int16), t_sep.view().view(torch.int16)), (t_ch.view().float() - t_sep.view().float()).abs().max().item()


@pytest.mark.parametrize("tile,cout", [(31, 128), (32, 64), (33, 32), (35, 64), (37, 128)])
def test_halo4_3x3_kernel_logic(sim, tile, cout):
    """conv3x3_halo.hip (4-wave LDS-halo kernel)"""
    _run_conv(sim, torch.float16, tile, 2, 64, cout, 11, 9, 3, 1, residual=True, seed=tile)


@pytest.mark.parametrize("tile,cout", [(111, 128), (112, 64), (114, 32), (116, 128), (115, 256)])
def test_igemm8_kernel_logic(sim, tile, cout):
    """conv_igemm8.hip (8 waves, 64-deep steps): pointwise and strided 3x3 forms"""
    _run_conv(sim, torch.float16, tile, 2, 64, cout, 10, 13, 1, 1, seed=tile)
    _run_conv(sim, torch.bfloat16, tile, 1, 64, cout, 12, 10, 3, 2, seed=tile + 1)


@pytest.mark.parametrize("tile,k", [(21, 1), (61, 1), (111, 1), (115, 3), (91, 3), (31, 3), (142, 1)])
def test_cout_96_and_192_take_the_lean_epilogue_and_equal_the_padded_convolution(sim, tile, k):
    """round 4: a wave tile whose trailing 16-channel packet pairs lie completely past cout (cout = 96 / 192 in a 128-wide block, 48 in a 64-wide one: yolov5m's widths; 80, 16)
    runs the lean epilogue for the packets inside -- until then every such wave tile went through the general one.  Against torch (inside _run_conv, neighbours of the output slice untouched), with and
    without a shortcut, both 16-bit types; and BIT-IDENTICAL to the first 96 / 192 channels of the same convolution zero-padded to 128 / 256 couts (whole wave tiles: the path
    that was lean before)"""
    from yolort_amd import engine
    for dtype, cout, res in [(torch.float16, 96, False), (torch.bfloat16, 96, True), (torch.float16, 192, True), (torch.bfloat16, 48, True), (torch.float16, 80, False), (torch.float16, 16, True)]:
        n, cin, h, w, s_ = 2, 64, 9, 11, 1
        got = _run_conv(sim, dtype, tile, n, cin, cout, h, w, k, s_, residual=res, seed=tile + cout)
        # the same operands (same generator stream as _run_conv), weights and bias zero-padded to the next multiple of 128
        g = torch.Generator().manual_seed(tile + cout)
        p = k // 2
        x = torch.randn(n, cin, h, w, generator=g).to(dtype).float()
        wt = (torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)).to(dtype).float()
        bias = torch.randn(cout, generator=g) * 0.1
        cp = (cout + 127) // 128 * 128
        wt_p, bias_p = torch.zeros(cp, cin, k, k), torch.zeros(cp)
        wt_p[:cout], bias_p[:cout] = wt, bias
        pc = engine.PackedConv(wt_p, bias_p, None, dtype, torch.device("cpu"))
        xb = Buf(n, h, w, cin, dtype, fill=x.permute(0, 2, 3, 1))
        yb = Buf(n, h, w, cp, dtype)
        rb = None
        if res:
            r = torch.randn(n, cout, h, w, generator=g).to(dtype).float()
            r_p = torch.zeros(n, cp, h, w)
            r_p[:, :cout] = r
            rb = Buf(n, h, w, cp, dtype, fill=r_p.permute(0, 2, 3, 1))
        d = _conv_desc(xb, pc, yb, tile, k=k, pad=p, res=rb, stride=s_)
        if k > 1:
            kt = pc.ktab(w, xb.cs)
            d.ktab = kt.data_ptr()
        _check(sim, sim.sim_conv2d(C.byref(d)))
        assert torch.equal(yb.view()[..., :cout].contiguous().view(torch.int16), got.contiguous().view(torch.int16)), (dtype, cout, res)


@pytest.mark.parametrize("tile,cout", [(12, 64), (21, 128), (24, 128), (27, 64), (61, 128), (64, 128), (66, 128)])
def test_igemm_v2_kernel_logic(sim, tile, cout):
    """conv_igemm_impl.hpp (4-wave LDS-DMA implicit GEMM): the tiles the yolov5s table uses, 1x1 / 3x3 / strided 3x3"""
    _run_conv(sim, torch.float16, tile, 2, 64, cout, 10, 13, 1, 1, residual=True, seed=tile)
    _run_conv(sim, torch.float16, tile, 1, 32, cout, 12, 10, 3, 2, seed=tile + 1)
    _run_conv(sim, torch.bfloat16, tile, 1, 64, cout, 9, 9, 3, 1, seed=tile + 2)


@pytest.mark.parametrize("tile,base,cout", [(141, 12, 64), (142, 21, 128), (143, 66, 128), (144, 61, 128), (151, 111, 128), (152, 112, 64), (155, 115, 256)])
def test_row_transposed_store_tiles_equal_their_base_tiles(sim, tile, base, cout):
    """StoreEpilogueTP (tiles 141-145 / 151-155: opt-in, written at the end of round 2): the same bits as the tile they derive from, through
    ragged pixel counts (partial last rows), a residual, pointwise and 3x3 forms, both 16-bit types"""
    for dtype, (n, cin, h, w, k, s_, res) in [(torch.float16, (2, 64, 10, 13, 1, 1, True)), (torch.bfloat16, (1, 64, 9, 9, 3, 1, False)),
                                             (torch.float16, (1, 32, 12, 10, 3, 2, False))]:
        a = _run_conv(sim, dtype, base, n, cin, cout, h, w, k, s_, residual=res, seed=tile)
        b = _run_conv(sim, dtype, tile, n, cin, cout, h, w, k, s_, residual=res, seed=tile)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_row_transposed_store_tile_with_channel_split(sim):
    """a fused cv1 + cv2 launch through a row-transposed tile: the wave tiles on either side of the split go to their own views"""
    from yolort_amd import engine
    dtype, cpu = torch.float16, torch.device("cpu")
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 128, 9, 11, generator=g).to(dtype).float()
    wt = (torch.randn(128, 128, 1, 1, generator=g) / 11).to(dtype).float()
    bias = torch.randn(128, generator=g) * 0.1
    pc = engine.PackedConv(wt, bias, None, dtype, cpu)
    xb = Buf(2, 9, 11, 128, dtype, fill=x.permute(0, 2, 3, 1))
    outs = []
    for tile in (21, 142):
        y1, cat = Buf(2, 9, 11, 64, dtype), Buf(2, 9, 11, 128, dtype)
        _check(sim, sim.sim_conv2d(C.byref(_conv_desc(xb, pc, y1, tile, y2=cat.slice_c(64, 64), split=64))))
        outs.append((y1.view().clone(), cat.view().clone()))
    ref = F.silu(F.conv2d(x, wt, bias)).permute(0, 2, 3, 1)
    assert (outs[1][0].float() - ref[..., :64]).abs().max().item() <= 2e-3 * max(1.0, ref.abs().max().item())
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)) and torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))
    assert outs[1][1].float()[..., :64].abs().max().item() == 0


@pytest.mark.parametrize("tile,base", [(142, 21), (143, 66), (144, 61)])
def test_row_transposed_store_tiles_write_the_upsampled_copy_as_whole_rows(sim, tile, base):
    """round 4: y2_mode 1 (the PAN's nn.Upsample folded into its producer) through StoreEpilogueTP -- the 2 x 2 copies leave as whole 64 TN-byte rows instead of four scattered
    32-byte pieces per packet; output and upsampled copy equal the base tile's bit for bit, the neighbouring channels of the concat buffer stay untouched, ragged pixel counts"""
    from yolort_amd import engine
    dtype, cpu = torch.float16, torch.device("cpu")
    g = torch.Generator().manual_seed(tile)
    n, cin, cout, h, w = 2, 64, 128, 7, 9
    x = torch.randn(n, cin, h, w, generator=g).to(dtype).float()
    wt = (torch.randn(cout, cin, 1, 1, generator=g) / 8).to(dtype).float()
    bias = torch.randn(cout, generator=g) * 0.1
    pc = engine.PackedConv(wt, bias, None, dtype, cpu)
    xb = Buf(n, h, w, cin, dtype, fill=x.permute(0, 2, 3, 1))
    outs = []
    for t in (base, tile):
        y, cat = Buf(n, h, w, cout, dtype), Buf(n, 2 * h, 2 * w, cout + 64, dtype)
        d = _conv_desc(xb, pc, y, t, y2=cat.slice_c(32, cout), split=0)
        d.y2_mode = 1
        _check(sim, sim.sim_conv2d(C.byref(d)))
        outs.append((y.view().clone(), cat.view().clone()))
    ref = F.silu(F.conv2d(x, wt, bias)).permute(0, 2, 3, 1)
    assert (outs[1][0].float() - ref).abs().max().item() <= 2e-3 * max(1.0, ref.abs().max().item())
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)) and torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))
    up = outs[1][1]
    assert torch.equal(up[:, ::2, ::2, 32:32 + cout], outs[1][0]) and torch.equal(up[:, 1::2, 1::2, 32:32 + cout], outs[1][0])
    assert up.float()[..., :32].abs().max().item() == 0 and up.float()[..., 32 + cout:].abs().max().item() == 0


def _sim_letterbox(sim, imgs, size, out_dtype, c_out=4, div=32):
    """the product's host recipe (YOLOTransform.geometry: reference transform.py:53-97, 297-330) + ymi_letterbox on the simulator"""
    from yolort_amd._lib import YMI_U8_HWC, dtype_code
    from yolort_amd.models.transform import YOLOTransform
    tr = YOLOTransform(size, size, size_divisible=div)
    (hb, wb), sizes, pads = tr.geometry([tr.image_hw(im) for im in imgs])
    n = len(imgs)
    imgs = [im.contiguous() for im in imgs]
    ptrs = (C.c_void_p * n)(*[im.data_ptr() for im in imgs])
    geom = (C.c_int32 * (6 * n))()
    for i, im in enumerate(imgs):
        h_in, w_in = tr.image_hw(im)
        geom[6 * i: 6 * i + 6] = [h_in, w_in, sizes[i][0], sizes[i][1], pads[i][0], pads[i][1]]
    out = torch.full((n, hb, wb, c_out), 7.0, dtype=out_dtype)
    in_code = YMI_U8_HWC if tr.is_hwc(imgs[0]) else dtype_code(imgs[0].dtype)
    _check(sim, sim.ymi_letterbox(ptrs, geom, n, in_code, out.data_ptr(), hb, wb, c_out, dtype_code(out_dtype), C.c_float(tr.fill_color), None))
    return out, sizes


@pytest.mark.parametrize("kernel", ["default", "pixel", "1", "2", "4"])
def test_letterbox_kernels_vs_oracle(sim, kernel, monkeypatch):
    """csrc/preproc_pool.hip on the simulator against the oracle's letterbox (reference transform.py:53-97, 297-330): every kernel variant,
    the rounding-trap shapes, fp32 / fp16 output, uint8 planar and interleaved input"""
    from oracle import yolov5_oracle as O
    from workloads.synth import synth_images
    monkeypatch.delenv("YOLORT_AMD_LETTERBOX", raising=False)
    monkeypatch.delenv("YOLORT_AMD_LB_BLOCKS", raising=False)
    if kernel != "default":
        monkeypatch.setenv("YOLORT_AMD_LETTERBOX", kernel.split("+")[0])
    if "+" in kernel:   # the persistent kernel with few blocks: every block walks several tiles (both staging buffers, tiles of different images)
        monkeypatch.setenv("YOLORT_AMD_LB_BLOCKS", kernel.split("+")[1][0])
    shapes = [(135, 101), (60, 80), (90, 160), (47, 63), (100, 37), (81, 60)]
    imgs = [synth_images(1, h, w, seed=h + w)[0] for h, w in shapes]
    ref, sizes = O.letterbox(imgs, 96, 96, 32)
    got, got_sizes = _sim_letterbox(sim, imgs, 96, torch.float32)
    assert got_sizes == sizes and tuple(got.shape[1:3]) == tuple(ref.shape[2:])
    assert (got[..., :3].permute(0, 3, 1, 2) - ref).abs().max().item() <= 5e-5 and got[..., 3].abs().max().item() == 0
    got16, _ = _sim_letterbox(sim, imgs, 96, torch.float16)
    assert (got16[..., :3].float().permute(0, 3, 1, 2) - ref).abs().max().item() <= 1e-3
    gotb, _ = _sim_letterbox(sim, imgs, 96, torch.bfloat16)   # bf16 output: pair conversion in the tiled kernels, software rounding in the per-pixel one -- the same bits
    assert (gotb[..., :3].float().permute(0, 3, 1, 2) - ref).abs().max().item() <= 8e-3
    monkeypatch.setenv("YOLORT_AMD_LETTERBOX", "pixel")
    refb, _ = _sim_letterbox(sim, imgs, 96, torch.bfloat16)
    assert torch.equal(gotb.view(torch.int16), refb.view(torch.int16))
    monkeypatch.delenv("YOLORT_AMD_LETTERBOX", raising=False)
    if kernel != "default":
        monkeypatch.setenv("YOLORT_AMD_LETTERBOX", kernel.split("+")[0])
    u8 = [(im * 255).round().to(torch.uint8) for im in imgs]
    ref8, _ = O.letterbox([u.float() / 255.0 for u in u8], 96, 96, 32)
    got8, _ = _sim_letterbox(sim, u8, 96, torch.float32)
    assert (got8[..., :3].permute(0, 3, 1, 2) - ref8).abs().max().item() <= 5e-5
    hwc8, _ = _sim_letterbox(sim, [u.permute(1, 2, 0).contiguous() for u in u8], 96, torch.float32)
    assert torch.equal(hwc8, got8)   # the interleaved ingest equals the planar one bit for bit


def test_letterbox_tile_whose_columns_map_to_one_uint8_source_column(sim, monkeypatch):
    """an up-scaled uint8 planar image whose resized region ends one column into a 128-column tile ((pl + wr - 1) % 128 == 0): the tile
    stages ONE source column (span 1, one 16-byte chunk per staged row) -- the chunk -> (row, column) reciprocal wrapped to 0 there and only
    plane 0 / row 0 was staged.  The tiled kernel must equal the per-pixel kernel bit for bit."""
    from yolort_amd._lib import dtype_code
    g = torch.Generator().manual_seed(5)
    outs = {}
    for knob in ("default", "pixel", "1"):
        monkeypatch.delenv("YOLORT_AMD_LETTERBOX", raising=False)
        if knob != "default":
            monkeypatch.setenv("YOLORT_AMD_LETTERBOX", knob)
        for hin, win, hr, wr, pt, pl, hb, wb in [(8, 65, 16, 129, 0, 0, 32, 160), (9, 33, 27, 257, 3, 0, 32, 288), (5, 40, 10, 125, 2, 4, 32, 160)]:
            im = torch.randint(0, 256, (3, hin, win), generator=torch.Generator().manual_seed(hin * win), dtype=torch.uint8).contiguous()
            ptrs = (C.c_void_p * 1)(im.data_ptr())
            geom = (C.c_int32 * 6)(hin, win, hr, wr, pt, pl)
            out = torch.full((1, hb, wb, 4), 7.0, dtype=torch.float32)
            _check(sim, sim.ymi_letterbox(ptrs, geom, 1, dtype_code(torch.uint8), out.data_ptr(), hb, wb, 4, dtype_code(torch.float32), C.c_float(114.0), None))
            outs.setdefault(knob, []).append(out)
    for a, b, c in zip(outs["default"], outs["pixel"], outs["1"]):
        assert torch.equal(a, b) and torch.equal(c, b)


def test_letterbox_identity_sizes_are_exact(sim):
    from oracle import yolov5_oracle as O
    from workloads.synth import synth_images
    imgs = [synth_images(1, 64, 96, seed=70 + i)[0] for i in range(3)]
    ref, _ = O.letterbox(imgs, 96, 96, 32)
    got, _ = _sim_letterbox(sim, imgs, 96, torch.float32)
    assert torch.equal(got[..., :3].permute(0, 3, 1, 2), ref)


@pytest.mark.parametrize("spp_g", ["default", "1"])
def test_spp_pool_and_upsample_exact(sim, spp_g, monkeypatch):
    """the SPP max-pool cascade (reference common.py:183-187) and the nearest x2 upsample (path_aggregation_network.py:123) are exact"""
    monkeypatch.delenv("YOLORT_AMD_SPP_G", raising=False)
    if spp_g != "default":
        monkeypatch.setenv("YOLORT_AMD_SPP_G", spp_g)
    from yolort_amd._lib import YMI_F16
    x = torch.randn(2, 64, 20, 17, generator=torch.Generator().manual_seed(7)).half()
    buf = Buf(2, 20, 17, 256, torch.float16)
    buf.view()[..., :64] = x.permute(0, 2, 3, 1)
    _check(sim, sim.ymi_spp_pool(buf.ptr, 2, 20, 17, 64, 256, YMI_F16, None))
    got = buf.view().float().permute(0, 3, 1, 2)
    for i, k in enumerate((5, 9, 13)):
        assert torch.equal(got[:, 64 * (i + 1): 64 * (i + 2)], F.max_pool2d(x.float(), k, 1, k // 2)), f"maxpool{k} not exact"
    if spp_g == "default":   # a 40x40 map (yolov5m / l at 1280x1280): four channel groups do not fit twice in LDS -> two groups (32-byte runs) per block
        x4 = torch.randn(1, 32, 40, 40, generator=torch.Generator().manual_seed(8)).half()
        b4 = Buf(1, 40, 40, 128, torch.float16)
        b4.view()[..., :32] = x4.permute(0, 2, 3, 1)
        _check(sim, sim.ymi_spp_pool(b4.ptr, 1, 40, 40, 32, 128, YMI_F16, None))
        assert 100 * 1024 <= sim.sim_max_lds() <= 160 * 1024
        g4 = b4.view().float().permute(0, 3, 1, 2)
        for i, k in enumerate((5, 9, 13)):
            assert torch.equal(g4[:, 32 * (i + 1): 32 * (i + 2)], F.max_pool2d(x4.float(), k, 1, k // 2)), f"40x40 maxpool{k} not exact"
    # bfloat16 (round 4: the plane is held as order keys and reduced with packed unsigned maxima): negative values, zeros of both signs, repeated values, tiny and huge magnitudes
    from yolort_amd._lib import YMI_BF16
    xb = torch.randn(2, 32, 13, 21, generator=torch.Generator().manual_seed(9)) * torch.tensor([1e-30, 1.0, 3e4, 1e30]).repeat(8).view(1, 32, 1, 1)
    xb[0, :, 3:6, 4:9] = 0.0
    xb[0, :, 4, 5] = -0.0
    xb[1, 5] = -xb[1, 5].abs() - 1.0          # an all-negative plane
    xb = xb.to(torch.bfloat16)
    bb = Buf(2, 13, 21, 128, torch.bfloat16)
    bb.view()[..., :32] = xb.permute(0, 2, 3, 1)
    _check(sim, sim.ymi_spp_pool(bb.ptr, 2, 13, 21, 32, 128, YMI_BF16, None))
    gb = bb.view().float().permute(0, 3, 1, 2)
    assert torch.equal(gb[:, :32], xb.float()), "the input slice is left as it was"
    for i, k in enumerate((5, 9, 13)):
        assert torch.equal(gb[:, 32 * (i + 1): 32 * (i + 2)], F.max_pool2d(xb.float(), k, 1, k // 2)), f"bf16 maxpool{k} not exact"
    # fp32 mode (round 5: the LDS cascade replaces the direct 169-tap kernel wherever the plane fits): fp32 buffers, same exactness incl. an all-negative plane and a 40 x 40 map
    from yolort_amd._lib import YMI_F32
    for (n_, c_, h_, w_) in ((2, 16, 13, 21), (1, 8, 40, 40)):
        xf = torch.randn(n_, c_, h_, w_, generator=torch.Generator().manual_seed(10 + h_))
        xf[0, 3] = -xf[0, 3].abs() - 1.0
        bf = torch.zeros(n_, h_, w_, 4 * c_ + 8)
        bf[..., :c_] = xf.permute(0, 2, 3, 1)
        _check(sim, sim.ymi_spp_pool(bf.data_ptr(), n_, h_, w_, c_, 4 * c_ + 8, YMI_F32, None))
        gf = bf.permute(0, 3, 1, 2)
        assert torch.equal(gf[:, :c_], xf) and gf[:, 4 * c_:].abs().max().item() == 0
        for i, k in enumerate((5, 9, 13)):
            assert torch.equal(gf[:, c_ * (i + 1): c_ * (i + 2)], F.max_pool2d(xf, k, 1, k // 2)), f"fp32 maxpool{k} not exact"
    up = Buf(2, 40, 34, 96, torch.float16)
    _check(sim, sim.ymi_upsample2x(buf.ptr, 256, 2, 20, 17, 64, up.slice_c(32, 64).ptr, 96, YMI_F16, None))
    gu = up.view().float().permute(0, 3, 1, 2)
    assert torch.equal(gu[:, 32:96], F.interpolate(x.float(), scale_factor=2.0, mode="nearest")) and gu[:, :32].abs().max().item() == 0


def _rand_boxes(rng, n):
    xy = rng.random((n, 2), dtype=np.float32) * 300
    wh = rng.random((n, 2), dtype=np.float32) * 80 + 2
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


@pytest.mark.parametrize("n,ncls,ties", [(1, 1, False), (7, 3, False), (300, 5, True), (1000, 80, True), (2500, 2, True)])
def test_batched_nms_bit_exact_vs_oracle(sim, n, ncls, ties):
    """csrc/postprocess.hip on the simulator -- record packing, the radix sort passes, segment search, the wave64 ballot / shuffle
    greedy NMS and the kept-index emission -- against the oracle (stable score-descending order, strict >,
    class-aware, fp32 IoU): the kept indices are equal, ties and all"""
    from oracle import yolov5_oracle as O
    rng = np.random.default_rng(n + ncls)
    boxes = _rand_boxes(rng, n)
    scores = rng.random(n, dtype=np.float32)
    if ties:
        scores = np.round(scores, 2).astype(np.float32)
    labels = rng.integers(0, ncls, n).astype(np.int32)
    ref = O.batched_nms(torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(labels.astype(np.int64)), 0.45).numpy()
    keep = np.zeros(max(n, 1), np.int32)
    count = np.zeros(1, np.int32)
    ws = np.zeros(int(sim.ymi_nms_ws_bytes(n)), np.uint8)
    _check(sim, sim.ymi_batched_nms(boxes.ctypes.data, scores.ctypes.data, labels.ctypes.data, n, C.c_float(0.45), keep.ctypes.data, count.ctypes.data,
                                    ws.ctypes.data, ws.size, None))
    np.testing.assert_array_equal(keep[: int(count[0])].astype(np.int64), ref)


def _sim_nms(sim, case):
    """ymi_batched_nms on the simulator with a DIRTY workspace and pre-filled outputs -> (rc, keep, count)"""
    n = len(case["scores"])
    labels = case["labels"].astype(np.int32)
    keep, count = np.full(max(n, 1), -7, np.int32), np.full(1, -7, np.int32)
    ws = np.full(int(sim.ymi_nms_ws_bytes(n)), 0x7f, np.uint8)
    rc = sim.ymi_batched_nms(case["boxes"].ctypes.data, case["scores"].ctypes.data, labels.ctypes.data, n, C.c_float(case["thr"]), keep.ctypes.data, count.ctypes.data,
                             ws.ctypes.data, ws.size, None)
    return rc, keep, count


@pytest.mark.parametrize("name", _post_cases.NMS_CASES)
def test_batched_nms_adversarial_vs_oracle(sim, name):
    """The stand-alone NMS on inputs chosen against it (tests/_post_cases.py), same sizes as the GPU form of this test (tests/test_ops_gpu.py; nothing is shrunk:
    the 2 700-box grids take ~20 s each here): scores of both signs, signed zeros, infinities and subnormals (the sort key must order ALL floats, -0.0 == +0.0 a tie
    broken by index), segments that keep more than NMS_KCAP boxes (read back from the spill area), zero / negative areas and IoU == threshold under strict >,
    coordinates near +-1e6, segments of 63..129 candidates around the 64-lane step, 2..4097 equal scores (radix pass counts, stability), one class per box.
    Kept indices equal the oracle's, element for element; every case first proves from the oracle's result that it is not vacuous."""
    from oracle import yolov5_oracle as O
    case = _post_cases.nms_case(name)
    ref = O.batched_nms(torch.from_numpy(case["boxes"]), torch.from_numpy(case["scores"]), torch.from_numpy(case["labels"]), case["thr"]).numpy()
    per_class = _post_cases.assert_nms_case_is_not_vacuous(name, case, ref)
    print(f"{name}: n={len(case['scores'])} classes={len(per_class)} oracle keeps {len(ref)} (largest class {per_class.max()})")
    rc, keep, count = _sim_nms(sim, case)
    _check(sim, rc)
    np.testing.assert_array_equal(keep[: int(count[0])].astype(np.int64), ref)


def test_batched_nms_refuses_two_to_the_twenty_candidates(sim):
    """candidate indices share a 32-bit word with 12 bits of class: n = 2^20 is refused by name, before anything is launched (outputs untouched); 2^20 - 1 is the limit"""
    n = 1 << 20
    case = dict(boxes=np.zeros((n, 4), np.float32), scores=np.zeros(n, np.float32), labels=np.zeros(n, np.int64), thr=0.45)
    rc, keep, count = _sim_nms(sim, case)
    assert rc != 0 and "out of range" in sim.sim_last_error().decode() and str(n - 1) in sim.sim_last_error().decode()
    assert int(count[0]) == -7 and (keep == -7).all()


@pytest.mark.parametrize("thr,k,saturated,cap0", [(0.3, 300, False, 4096), (0.05, 50, False, 4096), (0.3, 300, True, 4096), (0.02, 300, False, 131072), (0.3, 300, True, 131072),
                                                 (0.02, 300, "mixed", 131072), (0.005, 2000, False, 131072)])
def test_postprocess_vs_oracle(sim, thr, k, saturated, cap0):
    """ymi_postprocess on the simulator from the reference's own head-output layout: sigmoid / anchor decode, multi-label threshold, the
    per-image ranking sort, class-aware NMS, top-k and the in-kernel rescale (box_head.py:328-360, 414-427; transform.py:354-367) --
    counts, labels and order exact, scores / boxes to the rounding of expf.  cap0 = 131072: per-image regions of 65536 records, the MULTI-BLOCK form of the
    score-prefix selection (sel_hist / sel_compact / sel_copyback over four slices; the saturated image takes the refinement ladder, sel_rhist / sel_rpick).
    k = 2000: sel_t = 8000 lies past RANK_MAX, both images (about 32 k candidates each) walk the ladder to the exhausted key and keep exactly sel_t records, every one
    of which sel_copyback has to bring back (it used to be launched over RANK_MAX records per image: stale records in the sort, wrong detections, no status bit)"""
    from oracle import yolov5_oracle as O
    from yolort_amd._lib import PostDesc
    g = torch.Generator().manual_seed(11)
    n, nc = 2, 80
    kk = nc + 5
    shapes = [(10, 12), (5, 6), (3, 3)]
    heads = [torch.randn(n, 3, h, w, kk, generator=g) * 2.0 - 1.0 for h, w in shapes]
    if saturated == "mixed":   # multi-block selection with one crowded image (cut) and one sparse image (left alone) in the same batch
        for ho in heads:
            ho[1, ..., 4] -= 4.0
        saturated = False
        mixed = True
    else:
        mixed = False
    if saturated:
        # thousands of (anchor, class) pairs with scores within 1/4096 of 1.0 -- many exactly equal -- in image 0: the score-prefix selection's boundary
        # bin is FAT (round 3: refined by an exact radix selection on the full sort key instead of sending the image to the one-block sort)
        ho = heads[0]
        ho[0, :, :, :, 4] = 12.0 + torch.randn(ho[0, :, :, :, 4].shape, generator=g) * 0.3
        ho[0, :, :, :, 5:35] = 11.0 + torch.randn(ho[0, :, :, :, 5:35].shape, generator=g).round() * 0.5   # rounded: exact score ties
    strides, anchors = O.anchors_for(3)
    ref = O.postprocess(O.decode(heads, strides, anchors), thr, 0.45, k)
    rescale = torch.tensor([[0.5, 8.0, 0.0], [1.25, 0.0, 4.0]], dtype=torch.float32)   # {gain, pad_x, pad_y} per image (scale_coords)
    logits = []
    for ho in heads:
        cs = (3 * kk + 3) // 4 * 4
        t = torch.zeros(n, ho.shape[2], ho.shape[3], cs, dtype=torch.float32)
        t[..., : 3 * kk] = ho.permute(0, 2, 3, 1, 4).reshape(n, ho.shape[2], ho.shape[3], 3 * kk)
        logits.append(t)
    total_anchors = sum(3 * h * w for h, w in shapes)
    cap, flags = cap0, 0
    while True:   # the host protocol of yolort_amd/ops.py: nothing is truncated silently, a too small candidate capacity is grown and the batch redone
        boxes, scores = torch.zeros(n, k, 4), torch.zeros(n, k)
        labels, count, status = torch.zeros(n, k, dtype=torch.int64), torch.zeros(n, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
        slab = torch.full((n, 6 * k + 1), float("nan"))   # the packed wire slab the top-k kernel writes next to the four arrays (ymi_post_desc.out_slab, ABI 5)
        ws = torch.full((int(sim.ymi_postprocess_ws_bytes(n, total_anchors, cap)),), 0x7f, dtype=torch.uint8)   # a DIRTY workspace: nothing may rely on zeroed memory
        d = PostDesc()
        for i, (h, w) in enumerate(shapes):
            d.lh[i], d.lw[i], d.stride[i] = h, w, float(strides[i])
            for j in range(6):
                d.anchors[i][j] = float(anchors[i][j])
            d.logits[i], d.lcstride[i] = logits[i].data_ptr(), logits[i].shape[3]
        d.num_levels, d.n, d.num_classes = 3, n, nc
        d.score_thresh, d.nms_thresh, d.detections_per_img = thr, 0.45, k
        d.rescale = rescale.data_ptr()
        d.out_boxes, d.out_scores, d.out_labels, d.out_count = boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), count.data_ptr()
        d.status, d.ws, d.ws_bytes, d.cand_cap, d.flags = status.data_ptr(), ws.data_ptr(), ws.numel(), cap, flags
        d.out_slab = slab.data_ptr()
        _check(sim, sim.ymi_postprocess(C.byref(d), None))
        st = status.tolist()
        assert st[5] == n, st                                        # every block of the top-k kernel checked in (the last one fixes the slab up)
        if st[1] != 0:                                               # the host will redo this batch: every row of the slab says so (dist.SLAB_STALE)
            assert torch.equal(slab[:, 6 * k], torch.full((n,), -1.0)), slab[:, 6 * k]
        else:                                                        # the kernel-written slab IS pack_slab of the four arrays, slots past the count zeroed
            from yolort_amd import dist as ydist
            want = ydist.pack_slab(boxes, scores, labels, count)
            for i in range(n):
                c = int(count[i])
                for lo_, w_ in ((0, 4), (4 * k, 1), (5 * k, 1)):
                    assert torch.equal(slab[i, lo_: lo_ + w_ * c], want[i, lo_: lo_ + w_ * c]), (i, lo_)
                    assert float(slab[i, lo_ + w_ * c: lo_ + w_ * k].abs().sum()) == 0.0, (i, lo_)
                assert float(slab[i, 6 * k]) == c
            assert st[4] >= st[0] > 0, st                            # raw candidates of the batch >= the records that were sorted (score-prefix selection)
        if st[1] == 0:
            if cap0 > 4096 and mixed:
                assert 4096 <= st[0] <= 6144 + 6144 and len(ref[1]["scores"]) > 0, st   # image 0 cut to just above sel_t, image 1 (fewer than 1.5 sel_t records) untouched
            elif cap0 > 4096 and not saturated:
                sel_t = max(4 * k, 4096)
                assert 2 * sel_t <= st[0] <= 2 * max(6144, sel_t), st   # both images were cut to just above sel_t records (exactly sel_t past RANK_MAX = 6144): the selection ran -- with 65536-record regions, in its multi-block form
            if saturated:
                assert flags == 0 and st[0] <= 6144 + 4096, st   # the prefix path held: image 0 was cut to <= RANK_MAX records, no exact-full redo
            break
        if not st[1] & 1:
            flags = 1   # YMI_POST_EXACT_FULL
            continue
        need = max(st[0], st[3] * n)
        cap = max(int(need * 1.25) + 1024, 2 * cap)
        cap = n * (1 << ((cap + n - 1) // n - 1).bit_length())
    for i, r in enumerate(ref):
        c = int(count[i])
        assert c == len(r["scores"])
        np.testing.assert_array_equal(labels[i, :c].numpy(), r["labels"].numpy())
        np.testing.assert_allclose(scores[i, :c].numpy(), r["scores"].numpy(), rtol=2e-6, atol=1e-7)
        gain, px, py = rescale[i].tolist()
        want = (r["boxes"] - torch.tensor([px, py, px, py])) / gain
        np.testing.assert_allclose(boxes[i, :c].numpy(), want.numpy(), rtol=1e-5, atol=2e-4)


def _sim_post(sim, heads, strides, anchors, nc, thr, k, cap0=4096, fill=0.0):
    """ymi_postprocess on the simulator from reference-layout head outputs under the host protocol of yolort_amd/ops.py (grow the capacity / take the exact full pass
    and redo).  Outputs are pre-filled with `fill`, the workspace is dirty.  -> (rc, dict of the output arrays) of the last pass"""
    from yolort_amd._lib import PostDesc
    n, kk = heads[0].shape[0], nc + 5
    shapes = [(ho.shape[2], ho.shape[3]) for ho in heads]
    logits = []
    for ho in heads:
        cs = (3 * kk + 3) // 4 * 4
        t = torch.zeros(n, ho.shape[2], ho.shape[3], cs, dtype=torch.float32)
        t[..., : 3 * kk] = ho.permute(0, 2, 3, 1, 4).reshape(n, ho.shape[2], ho.shape[3], 3 * kk)
        logits.append(t)
    total_anchors = sum(3 * h * w for h, w in shapes)
    cap, flags = cap0, 0
    while True:
        out = dict(boxes=torch.full((n, k, 4), fill), scores=torch.full((n, k), fill), labels=torch.full((n, k), int(fill), dtype=torch.int64),
                   count=torch.full((n,), int(fill), dtype=torch.int32), status=torch.full((8,), int(fill), dtype=torch.int32))
        ws = torch.full((int(sim.ymi_postprocess_ws_bytes(n, total_anchors, cap)),), 0x7f, dtype=torch.uint8)
        d = PostDesc()
        for i, (h, w) in enumerate(shapes):
            d.lh[i], d.lw[i], d.stride[i] = h, w, float(strides[i])
            for j in range(6):
                d.anchors[i][j] = float(anchors[i][j])
            d.logits[i], d.lcstride[i] = logits[i].data_ptr(), logits[i].shape[3]
        d.num_levels, d.n, d.num_classes = len(shapes), n, nc
        d.score_thresh, d.nms_thresh, d.detections_per_img = thr, 0.45, k
        d.out_boxes, d.out_scores, d.out_labels, d.out_count = out["boxes"].data_ptr(), out["scores"].data_ptr(), out["labels"].data_ptr(), out["count"].data_ptr()
        d.status, d.ws, d.ws_bytes, d.cand_cap, d.flags = out["status"].data_ptr(), ws.data_ptr(), ws.numel(), cap, flags
        rc = sim.ymi_postprocess(C.byref(d), None)
        st = out["status"].tolist()
        if rc != 0 or st[1] == 0:
            return rc, out
        if not st[1] & 1:
            flags = 1   # YMI_POST_EXACT_FULL
            continue
        need = max(st[0], st[3] * n)
        cap = max(int(need * 1.25) + 1024, 2 * cap)
        cap = n * (1 << ((cap + n - 1) // n - 1).bit_length())


def _assert_post_equals_oracle(out, ref, k, fill):
    """counts, labels, order exact; scores / boxes to the rounding of expf (the constants of test_postprocess_vs_oracle); nothing written past the counts"""
    for i, r in enumerate(ref):
        c = int(out["count"][i])
        assert c == len(r["scores"]), (i, c, len(r["scores"]))
        np.testing.assert_array_equal(out["labels"][i, :c].numpy(), r["labels"].numpy())
        np.testing.assert_allclose(out["scores"][i, :c].numpy(), r["scores"].numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(out["boxes"][i, :c].numpy(), r["boxes"].numpy(), rtol=1e-5, atol=1e-4)
        assert (out["scores"][i, c:] == fill).all() and (out["labels"][i, c:] == int(fill)).all() and (out["boxes"][i, c:] == fill).all(), f"image {i}: slots past the count were written"


@pytest.mark.parametrize("nc", _post_cases.POST_CLASS_COUNTS)
def test_postprocess_vs_oracle_class_counts(sim, nc):
    """decode + threshold + sort + NMS + top-k against O.decode + O.postprocess at the class counts where the decode changes shape: 1 (one label bit, the smallest
    legal count), 27 / 28 (both sides of an anchor padding), 80 / 81 (255 channels = one float4 pass per pixel / the first count that needs two), 91, 124 (the first the
    fused head refuses), 166 (3 * 171 = 513 channels: the first pixel wider than the 512-record wave buffer), 200 and 601 (a pixel passes 600 / 1803 records: the buffer is
    flushed in the middle of a pixel).  Three images on the levels test_postprocess_vs_oracle uses here ((10, 12), (5, 6), (3, 3): a quarter of the GPU test's pixels);
    per class count a top-k cut at 7 with thousands of survivors and a batch whose middle image has no candidate; the other runs of the GPU test (cuts at 1 / 50 / 300,
    the threshold 0.3 on the full batch, a batch without any candidate) at nc = 2 only: a run costs ~15 s here whatever its size, the full list would take 20 minutes."""
    from oracle import yolov5_oracle as O
    shapes = [(10, 12), (5, 6), (3, 3)]
    strides, anchors = O.anchors_for(3)
    refs = {}
    for variant, thr, k, truncates in _post_cases.post_runs(nc, sum(3 * h * w for h, w in shapes), lean=True):
        heads = _post_cases.post_heads(nc, shapes, empty=_post_cases.POST_EMPTY[variant])
        if (variant, thr) not in refs:
            pred = O.decode(heads, strides, anchors)
            refs[variant, thr] = (pred, O.postprocess(pred, thr, 0.45, 1 << 30))
        pred, full = refs[variant, thr]
        survivors, hot = _post_cases.assert_post_case_is_not_vacuous(nc, variant, thr, k, truncates, pred, shapes, full)
        print(f"nc={nc} {variant} thr={thr} k={k}: candidates {_post_cases.oracle_candidates_per_anchor(pred, thr).sum(1).tolist()} survivors {survivors} hottest pixel {hot}")
        rc, out = _sim_post(sim, heads, strides, anchors, nc, thr, k, cap0=3 * 8192, fill=-3.0)
        _check(sim, rc)
        _assert_post_equals_oracle(out, [{key: v[:k] for key, v in r.items()} for r in full], k, -3.0)


def test_postprocess_batch_size_limit(sim):
    """1 025 images are refused by name BEFORE anything runs -- status words and outputs keep their pattern -- and 1 024 images (one 2 x 2 level, two classes) equal the oracle"""
    from oracle import yolov5_oracle as O
    strides, anchors = [8], [O.ANCHORS_P5[0]]
    g = torch.Generator().manual_seed(1025)
    rc, out = _sim_post(sim, [torch.randn(1025, 3, 1, 1, 7, generator=g) + 1.0], strides, anchors, 2, 0.3, 10, cap0=1025 * 64, fill=-3.0)
    assert rc != 0 and "1024" in sim.sim_last_error().decode(), sim.sim_last_error().decode()
    for key, v in out.items():
        assert (v == -3).all(), f"{key} was written although the batch was refused"
    heads = [torch.randn(1024, 3, 2, 2, 7, generator=g) + 1.0]
    ref = O.postprocess(O.decode(heads, strides, anchors), 0.3, 0.45, 10)
    rc, out = _sim_post(sim, heads, strides, anchors, 2, 0.3, 10, cap0=1024 * 64, fill=-3.0)
    _check(sim, rc)
    _assert_post_equals_oracle(out, ref, 10, -3.0)
    assert int(out["count"].sum()) > 1024


@pytest.mark.parametrize("dtype,nc", [(torch.float16, 80), (torch.bfloat16, 11)])
def test_fused_head_decode_equals_the_unfused_head(sim, dtype, nc):
    """conv_head_decode_group_kernel (head_decode.hpp: 1x1 head conv of box_head.py:74 with the sigmoid / anchor decode / multi-label threshold of
    :328-360, :418 in its epilogue, all levels in one launch) against the unfused form -- fp32 logits from the implicit GEMM, then decode_kernel --
    through the rest of the post-process: counts, labels, order, scores and boxes IDENTICAL.  Waves span two images at the 3x5 / 5x7 levels
    (the record buffer changes image mid-wave) and the threshold is low enough for the worklist to drain more than once per wave.  The per-wave
    worklist / record buffer hand data between lanes through LDS: on the simulator (lanes not in lockstep) this passes only with the wave
    fences of head_decode.hpp, and it passes under both lane orders (HIPSIM_REVERSE=1)."""
    from oracle import yolov5_oracle as O
    from yolort_amd import engine
    from yolort_amd._lib import ACT_NONE, PostDesc, dtype_code
    from yolort_amd.models.box_head import YOLOHead
    cpu = torch.device("cpu")
    g = torch.Generator().manual_seed(3 + nc)
    n, thr, k = 3, 0.05, 100
    chans, shapes = [32, 64, 96], [(12, 13), (5, 7), (3, 5)]
    head = YOLOHead(chans, 3, [8, 16, 32], nc).eval()
    kk = nc + 5
    with torch.no_grad():
        for m in head.head:
            m.weight.copy_((torch.randn(m.weight.shape, generator=g) * (1.5 / m.weight.shape[1] ** 0.5)).to(dtype).float())
            b = torch.zeros(3, kk)
            b[:, 4], b[:, 5:] = -1.5, -2.5
            m.bias.copy_(b.view(-1))
    feats = [torch.randn(n, c, h, w, generator=g).to(dtype).float() for c, (h, w) in zip(chans, shapes)]
    xs = [Buf(n, h, w, c, dtype, fill=f.permute(0, 2, 3, 1)) for f, c, (h, w) in zip(feats, chans, shapes)]
    strides, anchors = O.anchors_for(3)
    total_anchors = sum(3 * h * w for h, w in shapes)
    rescale = torch.tensor([[1.0, 0.0, 0.0]] * n, dtype=torch.float32)

    def post_desc(cap, logits=None):
        out = dict(boxes=torch.zeros(n, k, 4), scores=torch.zeros(n, k), labels=torch.zeros(n, k, dtype=torch.int64), count=torch.zeros(n, dtype=torch.int32),
                   status=torch.zeros(8, dtype=torch.int32), ws=torch.full((int(sim.ymi_postprocess_ws_bytes(n, total_anchors, cap)),), 0x7f, dtype=torch.uint8))
        d = PostDesc()
        for i, (h, w) in enumerate(shapes):
            d.lh[i], d.lw[i], d.stride[i] = h, w, float(strides[i])
            for j in range(6):
                d.anchors[i][j] = float(anchors[i][j])
            if logits is not None:
                d.logits[i], d.lcstride[i] = logits[i].data_ptr(), logits[i].shape[3]
        d.num_levels, d.n, d.num_classes = 3, n, nc
        d.score_thresh, d.nms_thresh, d.detections_per_img = thr, 0.45, k
        d.rescale = rescale.data_ptr()
        d.out_boxes, d.out_scores, d.out_labels, d.out_count = out["boxes"].data_ptr(), out["scores"].data_ptr(), out["labels"].data_ptr(), out["count"].data_ptr()
        d.status, d.ws, d.ws_bytes, d.cand_cap, d.flags = out["status"].data_ptr(), out["ws"].data_ptr(), out["ws"].numel(), cap, 1   # exact full pass: no score prefix
        return d, out

    cap = n * 16384
    # ---- unfused: fp32 logits (tile 21) + ymi_postprocess ----
    logits = []
    for i, (xb, (h, w)) in enumerate(zip(xs, shapes)):
        pc = head.packed(i, dtype, cpu, chans[i])
        cs = (3 * kk + 3) // 4 * 4
        lg = torch.zeros(n, h, w, cs, dtype=torch.float32)
        d = _conv_desc(xb, pc, Buf(n, h, w, 4, dtype), 21)
        d.y, d.y_cstride, d.act, d.out_dtype = lg.data_ptr(), cs, ACT_NONE, dtype_code(torch.float32)
        _check(sim, sim.sim_conv2d(C.byref(d)))
        logits.append(lg)
    d_ref, ref = post_desc(cap, logits)
    _check(sim, sim.ymi_postprocess(C.byref(d_ref), None))
    assert ref["status"].tolist()[1] == 0 and int(ref["count"].sum()) > 30
    # ---- fused: post_begin, ONE head launch for the three levels, post_finish ----
    from yolort_amd._lib import ConvDesc
    arr = (ConvDesc * 3)()
    keep = []
    for i, (xb, (h, w)) in enumerate(zip(xs, shapes)):
        pc = head.packed_anchor_major(i, dtype, cpu, chans[i])
        keep.append(pc)
        cd = _conv_desc(xb, pc, xb, 0)
        cd.y, cd.y_cstride, cd.act, cd.out_dtype = None, 0, ACT_NONE, dtype_code(torch.float32)
        C.memmove(C.byref(arr, i * C.sizeof(ConvDesc)), C.byref(cd), C.sizeof(ConvDesc))
    d_f, got = post_desc(cap)
    _check(sim, sim.ymi_post_begin(C.byref(d_f), None))
    _check(sim, sim.sim_conv_head_decode_group(arr, 3, C.byref(d_f)))
    _check(sim, sim.ymi_post_finish(C.byref(d_f), None))
    assert got["status"].tolist()[1] == 0
    assert torch.equal(got["count"], ref["count"])
    for key in ("labels", "scores", "boxes"):
        for i in range(n):
            c = int(ref["count"][i])
            assert torch.equal(got[key][i, :c], ref[key][i, :c]), (key, i)
    # and against the oracle's decode of the same logits: counts and labels exact
    heads = [lg[..., : 3 * kk].reshape(n, h, w, 3, kk).permute(0, 3, 1, 2, 4).contiguous() for lg, (h, w) in zip(logits, shapes)]
    want = O.postprocess(O.decode(heads, strides, anchors), thr, 0.45, k)
    for i, r in enumerate(want):
        c = int(got["count"][i])
        assert c == len(r["scores"])
        np.testing.assert_array_equal(got["labels"][i, :c].numpy(), r["labels"].numpy())


@pytest.mark.parametrize("name", list(_head_cases.SIM_SPECS))
def test_fused_head_equals_the_oracle_on_exact_logits(sim, name):
    """the simulator twin of tests/test_head_exact_gpu.py: conv_head_decode_group_kernel on inputs whose logits are exact (tests/_head_cases.py: one 1.0 per 32-channel block,
    weights exact in fp16 and bf16) through post_begin / post_finish against O.postprocess(O.decode(logits)) -- counts, labels, order exact, scores / boxes to the rounding of
    expf, nothing written past the counts.  sim-dense: a 32-pixel run across the image boundary passes more than HdCfg<1>::BUF = WL = 256 records per anchor (worklist spill,
    record-buffer flush, image change inside an append); sim-tie-below-quarter: scores of exactly 0.5 and 0.25 against the float below 0.25 (the pre-filter's margin decides
    the 0.25s); sim-thr-negative: every (anchor, class) pair passes, saturated logits included.  nms_thresh = 1.0 and k above the counts: the box of every candidate is
    compared.  Passes under both lane orders (HIPSIM_REVERSE=1)."""
    from yolort_amd._lib import ACT_NONE, ConvDesc, PostDesc, dtype_code
    case, want = _head_cases.head_case(name), _head_cases.head_reference(name)
    print(_head_cases.assert_head_case_is_not_vacuous(case, want))
    cpu, dtype, n, k, fill = torch.device("cpu"), case["dtype"], case["n"], case["k"], -3.0
    head = _head_cases.make_head(case)
    shapes, nl = case["shapes"], len(case["shapes"])
    xs = [Buf(n, h, w, c, dtype, fill=torch.from_numpy(x)) for x, c, (h, w) in zip(case["x"], case["chans"], shapes)]
    total_anchors, cap = sum(3 * h * w for h, w in shapes), case["cand_cap"]
    out = dict(boxes=torch.full((n, k, 4), fill), scores=torch.full((n, k), fill), labels=torch.full((n, k), int(fill), dtype=torch.int64),
               count=torch.full((n,), int(fill), dtype=torch.int32), status=torch.full((8,), int(fill), dtype=torch.int32))
    ws = torch.full((int(sim.ymi_postprocess_ws_bytes(n, total_anchors, cap)),), 0x7f, dtype=torch.uint8)   # a dirty workspace
    d = PostDesc()
    for i, (h, w) in enumerate(shapes):
        d.lh[i], d.lw[i], d.stride[i] = h, w, float(case["strides"][i])
        for j in range(6):
            d.anchors[i][j] = float(case["anchors"][i][j])
    d.num_levels, d.n, d.num_classes = nl, n, case["nc"]
    d.score_thresh, d.nms_thresh, d.detections_per_img = case["thr"], case["nms"], k
    d.out_boxes, d.out_scores, d.out_labels, d.out_count = out["boxes"].data_ptr(), out["scores"].data_ptr(), out["labels"].data_ptr(), out["count"].data_ptr()
    d.status, d.ws, d.ws_bytes, d.cand_cap, d.flags = out["status"].data_ptr(), ws.data_ptr(), ws.numel(), cap, 1   # exact full pass: no score prefix
    arr, keep = (ConvDesc * nl)(), []
    for i, xb in enumerate(xs):
        pc = head.packed_anchor_major(i, dtype, cpu, case["chans"][i])
        keep.append(pc)
        cd = _conv_desc(xb, pc, xb, 0)
        cd.y, cd.y_cstride, cd.act, cd.out_dtype = None, 0, ACT_NONE, dtype_code(torch.float32)
        C.memmove(C.byref(arr, i * C.sizeof(ConvDesc)), C.byref(cd), C.sizeof(ConvDesc))
    _check(sim, sim.ymi_post_begin(C.byref(d), None))
    _check(sim, sim.sim_conv_head_decode_group(arr, nl, C.byref(d)))
    _check(sim, sim.ymi_post_finish(C.byref(d), None))
    st = out["status"].tolist()
    assert st[1] == 0 and st[0] == int(case["cand"].sum()), st
    _assert_post_equals_oracle(out, want, k, fill)
    if case["expect_candidates"] is not None:
        assert int(out["count"].sum()) == case["expect_candidates"]
        assert all(torch.isin(out["scores"][i, : int(out["count"][i])], torch.tensor([0.25, 0.5, 1.0])).all() for i in range(n))


@pytest.mark.parametrize("cout,hw", [(32, (64, 96)), (48, (40, 64)), (16, (32, 64))])
def test_stem_kernels_logic(sim, cout, hw):
    """csrc/conv_stem.hip: Conv(3, c, k=6, s=2, p=2) (darknetv6.py:81) in its super-pixel form from the NHWC4 batch (tile 41) and straight
    from the planar images (the benchmark's op 0): both against torch, and equal to each other bit for bit"""
    from yolort_amd import engine
    from yolort_amd._lib import ACT_SILU, ConvDesc, dtype_code
    dtype, cpu = torch.float16, torch.device("cpu")
    g = torch.Generator().manual_seed(5 + cout)
    n, (h, w) = 2, hw
    x = torch.rand(n, 3, h, w, generator=g).to(dtype)
    wt = (torch.randn(cout, 3, 6, 6, generator=g) / 10).to(dtype).float()
    b = torch.randn(cout, generator=g) * 0.1
    ref = F.silu(F.conv2d(x.float(), wt, b, 2, 2)).permute(0, 2, 3, 1)
    pc = engine.PackedConv(wt, b, None, dtype, cpu, stem_superpixel=True)
    xb = Buf(n, h, w, 4, dtype)
    xb.view()[..., :3] = x.permute(0, 2, 3, 1)
    outs = []
    for planar in (False, True):
        yb = Buf(n, h // 2, w // 2, (cout + 7) // 8 * 8, dtype)
        d = ConvDesc()
        d.x, d.w, d.bias, d.y = xb.ptr, pc.w.data_ptr(), pc.bias.data_ptr(), yb.ptr
        d.n, d.h, d.w_in, d.cin, d.x_cstride = n, h, w // 2, 8, 8
        d.ho, d.wo, d.cout, d.cout_pad, d.y_cstride = h // 2, w // 2, cout, pc.cout_pad, yb.cs
        d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.k_pad = 6, 3, 2, 1, 2, 1, pc.k_pad
        d.act, d.dtype, d.out_dtype, d.tile = ACT_SILU, dtype_code(dtype), dtype_code(dtype), 41
        d.zeros = xb.zeros
        if planar:
            imgs = [x[i].contiguous() for i in range(n)]
            ptrs = (C.c_void_p * n)(*[im.data_ptr() for im in imgs])
            _check(sim, sim.sim_conv_stem_planar(C.byref(d), ptrs, n))
        else:
            _check(sim, sim.sim_conv2d(C.byref(d)))
        outs.append(yb.view()[..., :cout].clone())
        assert (outs[-1].float() - ref).abs().max().item() <= 2e-3 * max(1.0, ref.abs().max().item())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n,hw", [(1, (64, 64)), (2, (40, 104)), (1, (36, 72)), (2, (128, 160))])
def test_fused_stem_body1_equals_the_two_launches(sim, dtype, n, hw):
    """csrc/stem_body1_fused.hip: Conv(3, 32, 6, 2, 2) -> Conv(32, 64, 3, 2, 1) (darknetv6.py:81, :85-86) in one launch from the planar images,
    the stem's output living only in LDS -- BIT-IDENTICAL to conv_stem_planar_kernel followed by conv3x3_c32_kernel<2> (what the plan records
    for yolov5s), on sizes whose tiles are ragged in both directions and whose stem patch crosses the image border on every side"""
    from yolort_amd import engine
    from yolort_amd._lib import ACT_SILU, ConvDesc, dtype_code
    cpu = torch.device("cpu")
    if dtype == torch.bfloat16 and n * hw[0] * hw[1] > 10000:
        pytest.skip("the large case runs once (fp16)")
    g = torch.Generator().manual_seed(7 + hw[0])
    h, w = hw
    x = torch.rand(n, 3, h, w, generator=g).to(dtype)
    w0 = (torch.randn(32, 3, 6, 6, generator=g) / 8).to(dtype).float()
    b0 = torch.randn(32, generator=g) * 0.2
    w1 = (torch.randn(64, 32, 3, 3, generator=g) / 12).to(dtype).float()
    b1 = torch.randn(64, generator=g) * 0.2
    pc0 = engine.PackedConv(w0, b0, None, dtype, cpu, stem_superpixel=True)
    pc1 = engine.PackedConv(w1, b1, None, dtype, cpu)
    hs, ws = h // 2, w // 2
    ho, wo = (hs - 1) // 2 + 1, (ws - 1) // 2 + 1
    xb = Buf(n, h, w, 4, dtype)     # never read on the planar paths; its tail is the zero page
    imgs = [x[i].contiguous() for i in range(n)]
    ptrs = (C.c_void_p * n)(*[im.data_ptr() for im in imgs])

    def stem_desc(yb):
        d = ConvDesc()
        d.x, d.w, d.bias, d.y = xb.ptr, pc0.w.data_ptr(), pc0.bias.data_ptr(), yb.ptr
        d.n, d.h, d.w_in, d.cin, d.x_cstride = n, h, w // 2, 8, 8
        d.ho, d.wo, d.cout, d.cout_pad, d.y_cstride = hs, ws, 32, pc0.cout_pad, yb.cs
        d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.k_pad = 6, 3, 2, 1, 2, 1, pc0.k_pad
        d.act, d.dtype, d.out_dtype, d.tile = ACT_SILU, dtype_code(dtype), dtype_code(dtype), 41
        d.zeros = xb.zeros
        return d

    # ---- the two launches ----
    s_out = Buf(n, hs, ws, 32, dtype)
    _check(sim, sim.sim_conv_stem_planar(C.byref(stem_desc(s_out)), ptrs, n))
    y_sep = Buf(n, ho, wo, 64, dtype)
    kt = pc1.ktab(ws, 32)
    d1 = _conv_desc(s_out, pc1, y_sep, 131, k=3, pad=1, stride=2)
    d1.ktab = kt.data_ptr()
    _check(sim, sim.sim_conv2d(C.byref(d1)))
    # ---- one launch (into a channel slice of a wider buffer: nothing outside the slice is written) ----
    wide = Buf(n, ho, wo, 96, dtype)
    y_f = wide.slice_c(16, 64)
    dummy = Buf(n, hs, ws, 32, dtype)
    d1f = _conv_desc(dummy, pc1, y_f, 131, k=3, pad=1, stride=2)
    d1f.ktab = kt.data_ptr()
    _check(sim, sim.sim_stem_body1_planar(C.byref(stem_desc(dummy)), C.byref(d1f), ptrs, n))
    assert float(dummy.view().float().abs().max()) == 0.0            # the stem's output buffer is untouched
    got = y_f.view()
    assert torch.equal(got.view(torch.int16), y_sep.view().view(torch.int16)), f"max difference {(got.float() - y_sep.view().float()).abs().max().item()}"
    assert float(wide.view()[..., :16].float().abs().max()) == 0.0 and float(wide.view()[..., 80:].float().abs().max()) == 0.0
    # and against torch (two chained layers: twice the per-launch bound)
    mid = F.silu(F.conv2d(x.float(), w0, b0, 2, 2)).to(dtype).float()
    ref = F.silu(F.conv2d(mid, w1, b1, 2, 1)).permute(0, 2, 3, 1)
    tol = 4e-3 if dtype == torch.float16 else 3.2e-2
    assert (got.float() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n,hw", [(1, (64, 64)), (2, (40, 102)), (1, (36, 70)), (2, (96, 160))])
def test_fused_stem_body1_from_the_canvas_equals_the_two_launches(sim, dtype, n, hw):
    """the same kernel fed from the letterboxed NHWC4 canvas (dynamic-shape streams; ymi_stem_body1 / ymi_plan_set_fuse_stem): BIT-IDENTICAL to
    conv_stem_kernel (tile 41) followed by conv3x3_c32_kernel<2> (tile 131), on canvases whose width is NOT a multiple of 8 too"""
    from yolort_amd import engine
    from yolort_amd._lib import ACT_SILU, ConvDesc, dtype_code
    cpu = torch.device("cpu")
    if dtype == torch.bfloat16 and n * hw[0] * hw[1] > 10000:
        pytest.skip("the large case runs once (fp16)")
    g = torch.Generator().manual_seed(11 + hw[1])
    h, w = hw
    x = torch.rand(n, 3, h, w, generator=g).to(dtype)
    w0 = (torch.randn(32, 3, 6, 6, generator=g) / 8).to(dtype).float()
    b0 = torch.randn(32, generator=g) * 0.2
    w1 = (torch.randn(64, 32, 3, 3, generator=g) / 12).to(dtype).float()
    b1 = torch.randn(64, generator=g) * 0.2
    pc0 = engine.PackedConv(w0, b0, None, dtype, cpu, stem_superpixel=True)
    pc1 = engine.PackedConv(w1, b1, None, dtype, cpu)
    hs, ws = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    ho, wo = (hs - 1) // 2 + 1, (ws - 1) // 2 + 1
    canvas = torch.zeros(n, h, w, 4)
    canvas[..., :3] = x.float().permute(0, 2, 3, 1)
    xb = Buf(n, h, w, 4, dtype, fill=canvas)

    def stem_desc(yb):
        d = ConvDesc()
        d.x, d.w, d.bias, d.y = xb.ptr, pc0.w.data_ptr(), pc0.bias.data_ptr(), yb.ptr
        d.n, d.h, d.w_in, d.cin, d.x_cstride = n, h, w // 2, 8, 8
        d.ho, d.wo, d.cout, d.cout_pad, d.y_cstride = hs, ws, 32, pc0.cout_pad, yb.cs
        d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.k_pad = 6, 3, 2, 1, 2, 1, pc0.k_pad
        d.act, d.dtype, d.out_dtype, d.tile = ACT_SILU, dtype_code(dtype), dtype_code(dtype), 41
        d.zeros = xb.zeros
        return d

    s_out = Buf(n, hs, ws, 32, dtype)
    _check(sim, sim.sim_conv2d(C.byref(stem_desc(s_out))))
    y_sep = Buf(n, ho, wo, 64, dtype)
    kt = pc1.ktab(ws, 32)
    d1 = _conv_desc(s_out, pc1, y_sep, 131, k=3, pad=1, stride=2)
    d1.ktab = kt.data_ptr()
    _check(sim, sim.sim_conv2d(C.byref(d1)))
    y_f = Buf(n, ho, wo, 64, dtype)
    dummy = Buf(n, hs, ws, 32, dtype)
    d1f = _conv_desc(dummy, pc1, y_f, 131, k=3, pad=1, stride=2)
    d1f.ktab = kt.data_ptr()
    _check(sim, sim.sim_stem_body1(C.byref(stem_desc(dummy)), C.byref(d1f)))
    assert float(dummy.view().float().abs().max()) == 0.0            # the stem's output buffer is untouched
    got = y_f.view()
    assert torch.equal(got.view(torch.int16), y_sep.view().view(torch.int16)), f"max difference {(got.float() - y_sep.view().float()).abs().max().item()}"
    mid = F.silu(F.conv2d(x.float(), w0, b0, 2, 2)).to(dtype).float()
    ref = F.silu(F.conv2d(mid, w1, b1, 2, 1)).permute(0, 2, 3, 1)
    tol = 4e-3 if dtype == torch.float16 else 3.2e-2
    assert (got.float() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("k,s_,cin,cout", [(1, 1, 64, 96), (3, 1, 32, 40), (3, 2, 48, 64), (6, 2, 4, 32)])
def test_fp32_parity_kernel_logic(sim, k, s_, cin, cout):
    """csrc/conv_f32.hip (fp32 parity mode): exact fp32 arithmetic -- against torch's fp32 convolution to rounding-order accuracy"""
    from yolort_amd import engine
    from yolort_amd._lib import ACT_SILU, ConvDesc, YMI_F32
    g = torch.Generator().manual_seed(k * 10 + cin)
    n, h, w, p = 2, 13, 10, k // 2 if k != 6 else 2
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
    bias = torch.randn(cout, generator=g) * 0.1
    r = None
    ref = F.silu(F.conv2d(x, wt, bias, s_, p))
    ho, wo = ref.shape[2], ref.shape[3]
    pc = engine.PackedConv(wt, bias, None, torch.float32, torch.device("cpu"), cin_pad=(cin + 7) // 8 * 8)
    xb = torch.zeros(n, h, w, pc.cin)
    xb[..., :cin] = x.permute(0, 2, 3, 1)
    yb = torch.zeros(n, ho, wo, cout)
    d = ConvDesc()
    d.x, d.w, d.bias, d.y = xb.data_ptr(), pc.w.data_ptr(), pc.bias.data_ptr(), yb.data_ptr()
    kt = pc.ktab(w, pc.cin)
    d.ktab = kt.data_ptr()
    d.n, d.h, d.w_in, d.cin, d.x_cstride = n, h, w, pc.cin, pc.cin
    d.ho, d.wo, d.cout, d.cout_pad, d.y_cstride = ho, wo, cout, pc.cout_pad, cout
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.k_pad = k, k, s_, s_, p, p, pc.k_pad
    d.act, d.dtype, d.out_dtype, d.tile = ACT_SILU, YMI_F32, YMI_F32, -100
    _check(sim, sim.sim_conv2d(C.byref(d)))
    got = yb.permute(0, 3, 1, 2)
    assert (got - ref).abs().max().item() <= 2e-6 * max(1.0, ref.abs().max().item())


def _f32_desc(x_buf, pc, y, tile, k, s_, p, res=None, y2=None, split=0, up2=False, act=None):
    """fp32-mode conv descriptor over host NHWC fp32 buffers (x_buf: flat tensor with the 256-byte zero tail the plan buffers carry)"""
    from yolort_amd._lib import ACT_SILU, ConvDesc, YMI_F32
    xt, n, h, w, cs, tail = x_buf
    d = ConvDesc()
    d.x, d.w, d.bias, d.y = xt.data_ptr(), pc.w.data_ptr(), pc.bias.data_ptr(), y.data_ptr()
    kt = pc.ktab(w, cs)
    d.ktab = kt.data_ptr()
    d._keep = kt
    d.n, d.h, d.w_in, d.cin, d.x_cstride = n, h, w, pc.cin, cs
    ho, wo = (h + 2 * p - k) // s_ + 1, (w + 2 * p - k) // s_ + 1
    d.ho, d.wo, d.cout, d.cout_pad, d.y_cstride = ho, wo, pc.cout, pc.cout_pad, y.shape[-1]
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.k_pad = k, k, s_, s_, p, p, pc.k_pad
    d.act, d.dtype, d.out_dtype, d.tile = ACT_SILU if act is None else act, YMI_F32, YMI_F32, tile
    d.zeros = xt.data_ptr() + 4 * tail
    if res is not None:
        d.res, d.res_cstride = res.data_ptr(), res.shape[-1]
    if y2 is not None:
        d.y2, d.y2_cstride, d.cout_split, d.y2_mode = y2.data_ptr(), y2.shape[-1], split, 1 if up2 else 0
    return d


@pytest.mark.parametrize("tile", [201, 202, 203, 204, 205, 206, 0])
@pytest.mark.parametrize("k,s_,cin,cout", [(1, 1, 64, 96), (1, 1, 40, 128), (3, 1, 32, 40), (3, 2, 48, 64), (3, 1, 24, 32), (6, 2, 4, 32), (1, 1, 16, 32), (1, 1, 8, 40)])
def test_fp32_pipelined_kernel_logic(sim, tile, k, s_, cin, cout):
    """csrc/conv_f32_pipe.hip (round 5: the fp32 mode's LDS-DMA pipelined tiles): every tile in its three operand forms (pointwise, uniform tap,
    im2col table) against torch's fp32 convolution to rounding-order accuracy, and against the register-staged kernel it replaces"""
    from yolort_amd import engine
    g = torch.Generator().manual_seed(k * 10 + cin + tile)
    n, h, w, p = 2, 13, 10, k // 2 if k != 6 else 2
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
    bias = torch.randn(cout, generator=g) * 0.1
    ref = F.silu(F.conv2d(x, wt, bias, s_, p))
    ho, wo = ref.shape[2], ref.shape[3]
    pc = engine.PackedConv(wt, bias, None, torch.float32, torch.device("cpu"), cin_pad=(cin + 7) // 8 * 8)
    numel = n * h * w * pc.cin
    xt = torch.zeros(numel + 64)
    xt[:numel].view(n, h, w, pc.cin)[..., :cin] = x.permute(0, 2, 3, 1)
    outs = []
    for t in (tile, -100):
        yb = torch.zeros(n, ho, wo, cout)
        d = _f32_desc((xt, n, h, w, pc.cin, numel), pc, yb, t, k, s_, p)
        _check(sim, sim.sim_conv2d(C.byref(d)))
        outs.append(yb.permute(0, 3, 1, 2))
    scale = max(1.0, ref.abs().max().item())
    assert (outs[0] - ref).abs().max().item() <= 2e-6 * scale
    # the same k pairs in the same order, the same 64-element partial sums: BIT-IDENTICAL to the kernel the reference-made goldens were validated with
    assert torch.equal(outs[0], outs[1]), f"max difference {(outs[0] - outs[1]).abs().max().item()}"


@pytest.mark.parametrize("tile", [201, 202, 206])
def test_fp32_pipelined_kernel_split_shortcut_upsample(sim, tile):
    """the fp32 tiles' epilogue features: channel split into a second view (C3.cv1 + cv2 in one launch, common.py:172-173), the Bottleneck shortcut added after
    the activation (common.py:115-116), and the x2-upsampled second output (path_aggregation_network.py:221-223) -- written into channel slices of wider buffers"""
    from yolort_amd import engine
    g = torch.Generator().manual_seed(tile)
    n, h, w, cin = 2, 9, 7, 32
    x = torch.randn(n, cin, h, w, generator=g)
    numel = n * h * w * cin
    xt = torch.zeros(numel + 64)
    xt[:numel].view(n, h, w, cin)[:] = x.permute(0, 2, 3, 1)
    xb = (xt, n, h, w, cin, numel)
    # (a) split: couts [0, 32) -> y (own buffer), [32, 64) -> channels [8, 40) of a 48-wide buffer
    wt = torch.randn(64, cin, 1, 1, generator=g) / np.sqrt(cin)
    bias = torch.randn(64, generator=g) * 0.1
    pc = engine.PackedConv(wt, bias, None, torch.float32, torch.device("cpu"), cin_pad=cin)
    ref = F.silu(F.conv2d(x, wt, bias)).permute(0, 2, 3, 1)
    y, wide = torch.zeros(n, h, w, 32), torch.zeros(n, h, w, 48)
    d = _f32_desc(xb, pc, y, tile, 1, 1, 0, y2=wide[..., 8:], split=32)
    d.y2_cstride = 48
    _check(sim, sim.sim_conv2d(C.byref(d)))
    assert (y - ref[..., :32]).abs().max().item() <= 2e-6 * ref.abs().max().item()
    assert (wide[..., 8:40] - ref[..., 32:]).abs().max().item() <= 2e-6 * ref.abs().max().item()
    assert wide[..., :8].abs().max().item() == 0 and wide[..., 40:].abs().max().item() == 0
    # (b) 3x3 with the shortcut
    wt3 = torch.randn(32, cin, 3, 3, generator=g) / np.sqrt(cin * 9)
    b3 = torch.randn(32, generator=g) * 0.1
    pc3 = engine.PackedConv(wt3, b3, None, torch.float32, torch.device("cpu"), cin_pad=cin)
    res = torch.randn(n, h, w, 32, generator=g)
    ref3 = F.silu(F.conv2d(x, wt3, b3, 1, 1)).permute(0, 2, 3, 1) + res
    y3 = torch.zeros(n, h, w, 32)
    _check(sim, sim.sim_conv2d(C.byref(_f32_desc(xb, pc3, y3, tile, 3, 1, 1, res=res))))
    assert (y3 - ref3).abs().max().item() <= 2e-6 * ref3.abs().max().item()
    # (c) the upsampled copy: channels [0, 32) of a (n, 2h, 2w, 40) buffer
    up = torch.zeros(n, 2 * h, 2 * w, 40)
    y4 = torch.zeros(n, h, w, 32)
    pc4 = engine.PackedConv(wt[:32], bias[:32], None, torch.float32, torch.device("cpu"), cin_pad=cin)
    d4 = _f32_desc(xb, pc4, y4, tile, 1, 1, 0, y2=up, up2=True)
    _check(sim, sim.sim_conv2d(C.byref(d4)))
    assert torch.equal(y4, y)
    assert torch.equal(up[..., :32], y4.repeat_interleave(2, 1).repeat_interleave(2, 2)) and up[..., 32:].abs().max().item() == 0


@pytest.mark.parametrize("act_name", ["hardswish", "leaky"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("residual", [False, True])
def test_legacy_activation_kernel(sim, act_name, dtype, residual):
    """csrc/preproc_pool.hip act_kernel / ymi_act: Hardswish (reference common.py:64-65, `Conv(version="r3.1")`) and LeakyReLU(0.1) (common.py:140, `BottleneckCSP.act`) as
    the launch that follows an r3.1 convolution run with YMI_ACT_NONE -- in place, over a channel-slice view, the Bottleneck shortcut added AFTER the activation
    (common.py:115-116).  fp32: bit for bit torch's own functions (same order of operations); 16-bit: torch's result on the same stored values, rounded once."""
    from yolort_amd._lib import ACT_HARDSWISH, ACT_LEAKY, dtype_code
    act, fn = (ACT_HARDSWISH, F.hardswish) if act_name == "hardswish" else (ACT_LEAKY, lambda t: F.leaky_relu(t, 0.1))
    g = torch.Generator().manual_seed(3)
    n, h, w, c, cs, off = 2, 7, 9, 24, 48, 16          # a 24-channel slice at offset 16 of a 48-channel buffer
    buf = (torch.randn(n, h, w, cs, generator=g) * 3.0).to(dtype)
    before = buf.clone()
    res = (torch.randn(n, h, w, 32, generator=g)).to(dtype) if residual else None
    es = buf.element_size()
    _check(sim, sim.ymi_act(buf.data_ptr() + off * es, cs, n * h * w, c, dtype_code(dtype), act, None if res is None else res.data_ptr() + 8 * es, 32, None))
    want = fn(before[..., off:off + c].float())
    if residual:
        want = want + res[..., 8:8 + c].float()
    got = buf[..., off:off + c]
    if dtype == torch.float32:
        assert torch.equal(got, want)
    else:
        assert torch.equal(got, want.to(dtype))
    assert torch.equal(buf[..., :off], before[..., :off]) and torch.equal(buf[..., off + c:], before[..., off + c:])   # nothing outside the slice is touched
    assert float((before[..., off:off + c].float() < -3).float().mean()) > 0.05 and float((before[..., off:off + c].float() > 3).float().mean()) > 0.05   # both clamps of the Hardswish are exercised


def test_layout_edges_and_view_copy(sim):
    """the module-level API edges (NCHW <-> NHWC view, fp32 <-> fp16) and the strided channel-slice copy are exact"""
    from yolort_amd._lib import YMI_F16, YMI_F32
    x = torch.randn(2, 13, 7, 9, generator=torch.Generator().manual_seed(3))
    nhwc = Buf(2, 7, 9, 24, torch.float16)                      # 13 channels padded to 16 inside a 24-wide buffer
    _check(sim, sim.ymi_nchw_to_nhwc(x.data_ptr(), 2, 13, 7, 9, YMI_F32, nhwc.slice_c(8, 16).ptr, 24, 16, YMI_F16, None))
    v = nhwc.view().float()
    assert torch.equal(v[..., 8:21], x.half().float().permute(0, 2, 3, 1)) and v[..., :8].abs().max().item() == 0 and v[..., 21:].abs().max().item() == 0
    back = torch.zeros(2, 13, 7, 9)
    _check(sim, sim.ymi_nhwc_to_nchw(nhwc.slice_c(8, 16).ptr, 24, 2, 13, 7, 9, YMI_F16, back.data_ptr(), YMI_F32, None))
    assert torch.equal(back, x.half().float())
    dst = Buf(2, 7, 9, 40, torch.float16)
    _check(sim, sim.ymi_copy_view(nhwc.slice_c(8, 16).ptr, 24, 2 * 7 * 9, 16, dst.slice_c(16, 16).ptr, 40, YMI_F16, None))
    d = dst.view().float()
    assert torch.equal(d[..., 16:32], v[..., 8:24]) and d[..., :16].abs().max().item() == 0 and d[..., 32:].abs().max().item() == 0


# ---------------------------------------------------------------------------------------------------------------------
# The strip kernel of a whole C3 / its Bottlenecks (csrc/c3_tile.hip, round 6): hidden widths 64 / 128, weights streamed
# through one LDS ring in MFMA fragment order (ymi_c3_pack).  BIT-IDENTICAL to the separate launches of the tiles the pinned
# plan records for these layers (1x1: any implicit-GEMM tile; 3x3: the 8-wave LDS-halo kernel), and close to torch fp32.
# ---------------------------------------------------------------------------------------------------------------------
def _make_c3_wide(c1, c2, n, shortcut, seed):
    from yolort_amd.v5.models.common import C3
    torch.manual_seed(seed)
    m = C3(c1, c2, n=n, shortcut=shortcut).eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.6, 1.4)
                mod.bias.normal_(0, 0.2)
                mod.running_mean.normal_(0, 0.3)
                mod.running_var.uniform_(0.5, 1.5)
    return m


def _c3_tile_desc(dtype, n, h, w, c_in, c_, shortcut, mode, pc12, pcm1, pcm2, pc3):
    from yolort_amd._lib import C3Desc, dtype_code
    d = C3Desc()
    d.n, d.h, d.w, d.dtype = n, h, w, dtype_code(dtype)
    d.c_in, d.c_hidden, d.c_out, d.n_bottlenecks, d.shortcut, d.mode = c_in, c_, 2 * c_, 1, 1 if shortcut else 0, mode
    if pc12 is not None:
        d.w12, d.b12, d.k12_pad = pc12.w.data_ptr(), pc12.bias.data_ptr(), pc12.k_pad
    d.wm1, d.bm1, d.km1_pad = pcm1.w.data_ptr(), pcm1.bias.data_ptr(), pcm1.k_pad
    d.wm2, d.bm2, d.km2_pad = pcm2.w.data_ptr(), pcm2.bias.data_ptr(), pcm2.k_pad
    if pc3 is not None:
        d.w3, d.b3, d.k3_pad = pc3.w.data_ptr(), pc3.bias.data_ptr(), pc3.k_pad
    return d


def _c3_pack(sim, d):
    nb = sim.ymi_c3_blob_bytes(C.byref(d))
    assert nb > 0
    blob = torch.zeros(nb + 16, dtype=torch.uint8)
    _check(sim, sim.ymi_c3_pack(C.byref(d), blob.data_ptr(), None))
    d.wblob = blob.data_ptr()
    return blob


def _run_c3_tile_case(sim, dtype, n, h, w, c_in, c_, nb, shortcut, t1x1=21, t3x3=91, blocks=None, geom=None):
    cpu = torch.device("cpu")
    m = _make_c3_wide(c_in, 2 * c_, nb, shortcut, seed=h * 7 + w + nb)
    x = torch.randn(n, c_in, h, w, generator=torch.Generator().manual_seed(n + h + c_)).to(dtype).float()
    xb = Buf(n, h, w, c_in, dtype, fill=x.permute(0, 2, 3, 1))
    pc12 = m.packed_pair(dtype, cpu, c_in)
    pc3 = m.cv3.packed(dtype, cpu, 2 * c_)
    pcs = [(b.cv1.packed(dtype, cpu, c_), b.cv2.packed(dtype, cpu, c_)) for b in m.m]

    # ---- the separate launches (what C3.emit records without the strip kernel) ----
    cat, out_sep = Buf(n, h, w, 2 * c_, dtype), Buf(n, h, w, 2 * c_, dtype)
    y = Buf(n, h, w, c_, dtype)
    _check(sim, sim.sim_conv2d(C.byref(_conv_desc(xb, pc12, y, t1x1, y2=cat.slice_c(c_, c_), split=c_))))
    for j, (pcm1, pcm2) in enumerate(pcs):
        t = Buf(n, h, w, c_, dtype)
        _check(sim, sim.sim_conv2d(C.byref(_conv_desc(y, pcm1, t, t1x1))))
        yo = cat.slice_c(0, c_) if j == nb - 1 else Buf(n, h, w, c_, dtype)
        _check(sim, sim.sim_conv2d(C.byref(_conv_desc(t, pcm2, yo, t3x3, k=3, pad=1, res=y if shortcut else None))))
        y = yo
    _check(sim, sim.sim_conv2d(C.byref(_conv_desc(cat, pc3, out_sep, t1x1))))

    # ---- the strip kernel: one launch (nb == 1) or HEAD, MID ..., TAIL ----
    if blocks is not None:
        os.environ["YOLORT_AMD_C3T_BLOCKS"] = str(blocks)
    if geom is not None:
        os.environ["YOLORT_AMD_C3T_GEOM"] = geom
    try:
        wide = Buf(n, h, w, 2 * c_ + 32, dtype)   # the output is a channel slice of a wider buffer
        out_f = wide.slice_c(16, 2 * c_)
        keep = []
        if nb == 1:
            d = _c3_tile_desc(dtype, n, h, w, c_in, c_, shortcut, 0, pc12, pcs[0][0], pcs[0][1], pc3)
            d.x, d.x_cstride, d.y, d.y_cstride = xb.ptr, xb.cs, out_f.ptr, out_f.cs
            assert sim.ymi_c3_tile_supported(C.byref(d)) == 1
            keep.append(_c3_pack(sim, d))
            _check(sim, sim.sim_c3_tile(C.byref(d)))
        else:
            cat_f = Buf(n, h, w, 2 * c_, dtype)
            y2v = cat_f.slice_c(c_, c_)
            ya, yb_ = Buf(n, h, w, c_, dtype), Buf(n, h, w, c_, dtype)
            d = _c3_tile_desc(dtype, n, h, w, c_in, c_, shortcut, 1, pc12, pcs[0][0], pcs[0][1], None)
            d.x, d.x_cstride = xb.ptr, xb.cs
            d.y1_out, d.y1_out_cstride, d.y2, d.y2_cstride = ya.ptr, ya.cs, y2v.ptr, y2v.cs
            keep.append(_c3_pack(sim, d))
            _check(sim, sim.sim_c3_tile(C.byref(d)))
            cur, nxt = ya, yb_
            for j in range(1, nb - 1):
                d = _c3_tile_desc(dtype, n, h, w, c_in, c_, shortcut, 2, None, pcs[j][0], pcs[j][1], None)
                d.y1_in, d.y1_in_cstride, d.y1_out, d.y1_out_cstride = cur.ptr, cur.cs, nxt.ptr, nxt.cs
                keep.append(_c3_pack(sim, d))
                _check(sim, sim.sim_c3_tile(C.byref(d)))
                cur, nxt = nxt, cur
            d = _c3_tile_desc(dtype, n, h, w, c_in, c_, shortcut, 3, None, pcs[nb - 1][0], pcs[nb - 1][1], pc3)
            d.y1_in, d.y1_in_cstride, d.y2, d.y2_cstride = cur.ptr, cur.cs, y2v.ptr, y2v.cs
            d.y, d.y_cstride = out_f.ptr, out_f.cs
            keep.append(_c3_pack(sim, d))
            _check(sim, sim.sim_c3_tile(C.byref(d)))
    finally:
        os.environ.pop("YOLORT_AMD_C3T_BLOCKS", None)
        os.environ.pop("YOLORT_AMD_C3T_GEOM", None)

    a, b = out_sep.view(), out_f.view()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"strip kernel vs separate launches: max difference {(a.float() - b.float()).abs().max().item()}"
    w_all = wide.view().float()
    assert w_all[..., :16].abs().max().item() == 0 and w_all[..., 16 + 2 * c_:].abs().max().item() == 0   # nothing outside the slice
    with torch.no_grad():
        x1, x2 = _torch_conv(m.cv1, x, dtype), _torch_conv(m.cv2, x, dtype)
        for bt in m.m:
            x1 = _torch_conv(bt.cv2, _torch_conv(bt.cv1, x1, dtype), dtype, res=x1 if shortcut else None)
        ref = _torch_conv(m.cv3, torch.cat([x1, x2], 1), dtype).permute(0, 2, 3, 1)
    tol = 4e-3 if dtype == torch.float16 else 3.2e-2
    err = (b.float() - ref).abs().max().item()
    assert err <= tol * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("case", [
    # (dtype, n, h, w, c_in, hidden, bottlenecks, shortcut, blocks)
    (torch.float16, 1, 40, 40, 256, 128, 1, False, None),    # yolov5s pan.layer_blocks.2: R = 5, eight strips, one centre group per wave
    (torch.float16, 2, 13, 40, 64, 128, 1, True, 3),         # a ragged last strip, the shortcut, three blocks walking six strips
    (torch.bfloat16, 1, 10, 40, 96, 128, 3, True, 1),        # HEAD, MID, TAIL (backbone.body.6's chain), ONE block: the ring runs across strips
    (torch.float16, 1, 12, 80, 128, 64, 1, False, None),     # 80 x 80 level: two centre groups per wave
    (torch.float16, 1, 9, 80, 64, 64, 2, True, 1),           # HEAD + TAIL (backbone.body.4's chain)
    (torch.bfloat16, 1, 7, 24, 64, 64, 1, True, None),       # a narrow map: many rows per strip
    (torch.float16, 1, 20, 20, 96, 128, 1, False, None),
])
def test_c3_strip_kernel_equals_the_separate_launches_and_torch(sim, case):
    dtype, n, h, w, c_in, c_, nb, shortcut, blocks = case
    _run_c3_tile_case(sim, dtype, n, h, w, c_in, c_, nb, shortcut, t3x3=91 if c_ == 128 else 92, blocks=blocks)


@pytest.mark.parametrize("case", [
    # (dtype, n, h, w, c_in, hidden, bottlenecks, shortcut, blocks, forced geometry "R,delta,column tiles" or None = the library's choice)
    (torch.float16, 1, 9, 60, 64, 128, 1, True, 2, "3,1,2"),       # two column tiles of 30 + a halo column either side; image edges left / right / between the tiles
    (torch.float16, 2, 10, 150, 64, 64, 2, True, 3, "4,1,3"),      # HEAD + TAIL over 3 x 50 columns, a ragged last row band, three blocks walk 18 tiles
    (torch.bfloat16, 1, 5, 200, 32, 128, 1, False, None, None),    # a 200-wide map at hidden 128: no full-width strip fits -- the library cuts columns by itself
    (torch.float16, 1, 6, 70, 64, 64, 1, False, 1, "2,3,4"),       # 4 tiles of 18 columns over 70 (the last one holds 16): ragged columns, one block
])
def test_c3_strip_kernel_with_column_tiles(sim, case):
    """maps wider than the LDS patch holds (yolov5l6 at 1280: hidden 64 @ 320 x 320, hidden 128 @ 160 x 160): a row band is cut into column tiles with one halo column either
    side (recomputed); results bit-identical to the separate launches, like the full-width strips"""
    dtype, n, h, w, c_in, c_, nb, shortcut, blocks, geom = case
    _run_c3_tile_case(sim, dtype, n, h, w, c_in, c_, nb, shortcut, t3x3=91 if c_ == 128 else 92, blocks=blocks, geom=geom)


# ---- per-element checks on exactly representable operands (tests/_exact.py): the CPU half of tests/test_conv_exact_gpu.py -------------------------------------------------
import _exact  # noqa: E402

# (the register-staged 16-bit kernel, tile 145 and the library rule are not part of the simulator build; every tile id runs on the GPU -- here the first and the last tile of
# each family in fp16 and other tiles of the same families in bf16: a lane-accurate launch costs tenths of a second)
_EXACT_SIM_FP16 = [12, 66, 111, 116, 31, 37, 91, 95, 121, 124, 141, 155, 131, 132, 133, 134, 135, 137, 138]
_EXACT_SIM_BF16 = [21, 61, 113, 34, 93, 122, 143, 152, 131, 132, 133, 134, 135, 138]


def _exact_sim_launch(sim, dtype, tile, case, act, residual):
    """one launch on exact operands; returns the (n, ho, wo, cout) output, or None when the kernel refused the shape with YMI_EINVAL (and wrote nothing)"""
    from yolort_amd import engine
    from yolort_amd._lib import ACT_NONE, ACT_SILU
    n, h, w, cin, cout, k, s = case
    x, wt, bias, res = _exact.exact_operands(*case)
    ho, wo = _exact.out_hw(h, w, k, s)
    cpu = torch.device("cpu")
    if dtype == torch.float32:
        pc = engine.PackedConv(wt.float(), bias.float(), None, dtype, cpu, cin_pad=cin)
        numel = n * h * w * cin
        xt = torch.zeros(numel + 64)
        xt[:numel].view(n, h, w, cin)[:] = x.permute(0, 2, 3, 1).float()
        wide_t = torch.zeros(n, ho, wo, cout + 32)
        rt = res.permute(0, 2, 3, 1).float().contiguous() if residual else None
        d = _f32_desc((xt, n, h, w, cin, numel), pc, wide_t[..., 16:16 + cout], tile, k, s, k // 2, res=rt, act=ACT_SILU if act else ACT_NONE)
        d.y_cstride = cout + 32
        got_view = wide_t[..., 16:16 + cout]
    else:
        pc = engine.PackedConv(wt.float(), bias.float(), None, dtype, cpu)
        xb = Buf(n, h, w, cin, dtype, fill=x.permute(0, 2, 3, 1))
        wide = Buf(n, ho, wo, cout + 32, dtype)           # the output is a channel slice of a wider buffer
        yv = wide.slice_c(16, cout)
        rb = Buf(n, ho, wo, cout, dtype, fill=res.permute(0, 2, 3, 1)) if residual else None
        d = _conv_desc(xb, pc, yv, tile, k=k, pad=k // 2, res=rb, stride=s)
        d.act = ACT_SILU if act else ACT_NONE
        if k > 1:
            kt = pc.ktab(w, xb.cs)
            d.ktab = kt.data_ptr()
        wide_t, got_view = wide.view(), yv.view()
    rc = sim.sim_conv2d(C.byref(d))
    if rc != 0:
        assert rc == -1, f"tile {tile} {case}: refusals carry YMI_EINVAL, got {rc}: {sim.sim_last_error().decode()}"
        assert float(wide_t.float().abs().max()) == 0, f"tile {tile} {case}: refused, yet something was written"
        return None
    w_all = wide_t.float()
    assert w_all[..., :16].abs().max().item() == 0 and w_all[..., 16 + cout:].abs().max().item() == 0, f"tile {tile} {case}: stray write outside the channel slice"
    return got_view.clone()


def _exact_sim_tile(sim, tile, dtype):
    """_exact.sim_cases(tile) in both activation modes (the large map of the general families: one of the two per launch): act none bit-identical to the once-rounded float64 reference (shortcut on every other case); SiLU within 1 ulp (the
    simulator's exp2f and 1/x are near-exact: off by one only next to a rounding tie) and |mean signed error| <= 0.1 ulp over the case"""
    tally = {0: _exact.Tally(), 1: _exact.Tally()}
    one_shape = _exact.family_of(tile) in ("c32", "res", "rw2", "rw3", "rs")
    for i, case in enumerate(_exact.sim_cases(tile)):
        # both modes on every small map; on the large map (the costly launches here: tenths of a second each) the general families take one mode, alternating from kind to kind and tile to tile
        for act in (0, 1) if (one_shape or _exact.group_of(case) == "small maps") else ((i + tile) % 2,):
            residual = (i // 2 + act) % 2 == 0 and not (act and tile in _exact.NO_SHORTCUT)
            got = _exact_sim_launch(sim, dtype, tile, case, act, residual)
            if got is None:
                tally[act].refused += 1
                continue
            ref = _exact.reference64(*case, bool(act), residual)
            label = f"tile {tile} {str(dtype)[6:]} {case} act={'silu' if act else 'none'} res={int(residual)}"
            tally[act].add(*_exact.assert_elementwise(got, ref, dtype, 1 if act else 0, label), label, _exact.group_of(case))
    for act in (0, 1):
        assert tally[act].ran > 0 or (act == 0 and tile in _exact.SILU_ONLY), f"tile {tile}: every case was refused"
        tally[act].verdict(f"sim tile {tile} {str(dtype)[6:]} act={'silu' if act else 'none'}")
    return tally


@pytest.mark.parametrize("tile", _EXACT_SIM_FP16)
def test_exact_operands_per_element_fp16(sim, tile):
    """every kernel family of the simulator build on exactly representable operands (tests/_exact.py: fp32 accumulation exact in any order), fp16 storage: 1x1 / 1xW / Hx1 maps,
    maps smaller than the window, ragged maps, 3x3 at both strides, one tap per output channel -- per element against the float64 reference rounded once"""
    _exact_sim_tile(sim, tile, torch.float16)


@pytest.mark.parametrize("tile", _EXACT_SIM_BF16)
def test_exact_operands_per_element_bf16(sim, tile):
    """the same in bf16 storage (the 8-bit significand makes almost every output a rounding, ties included)"""
    _exact_sim_tile(sim, tile, torch.bfloat16)


@pytest.mark.parametrize("tile", [201, 206])
def test_exact_operands_per_element_fp32(sim, tile):
    """fp32 mode (csrc/conv_f32_pipe.hip): exact operands leave nothing to round without an activation -- bit-identical; SiLU (expf, true
    division) within 1 ulp of fp32 of the float64 reference"""
    tally = {0: _exact.Tally(), 1: _exact.Tally()}
    for i, case in enumerate(_exact.cases(201, widths=[(32, 32), (48, 96)] if tile == 201 else [(64, 40)], shapes=_exact.SHAPES[:5])):
        for act in ((i + tile) % 2,):
            residual = (i // 2) % 2 == 0
            got = _exact_sim_launch(sim, torch.float32, tile, case, act, residual)
            assert got is not None, (tile, case)
            label = f"fp32 tile {tile} {case} act={act} res={int(residual)}"
            # SiLU + shortcut cancels, and the error of SiLU -- an ulp of ITS magnitude -- is many ulps of a small sum: the distance is measured at max(|SiLU|, |sum|), and the
            # bound is 1 + 1 (SiLU's ulp, then the addition's own rounding against the reference's single one)
            scale = _exact.reference64(*case, True, False) if (act and residual) else None
            tally[act].add(*_exact.assert_elementwise(got, _exact.reference64(*case, bool(act), residual), torch.float32, (2 if scale is not None else 1) if act else 0, label, scale64=scale),
                           label, _exact.group_of(case))
    for act in (0, 1):
        tally[act].verdict(f"sim fp32 tile {tile} act={act}")


@pytest.mark.parametrize("tile", [153, 154])
def test_exact_unknown_row_transposed_ids_are_refused(sim, tile):
    """the 15x range has no variants 13 / 14: refused with YMI_EINVAL, nothing written"""
    assert _exact_sim_launch(sim, torch.float16, tile, (2, 3, 3, 32, 32, 1, 1), 1, False) is None


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("act_name", ["hardswish", "leaky"])
def test_exact_legacy_activation_domain(sim, act_name, dtype):
    """ymi_act over the whole domain: every finite fp16 value / every finite bf16 value with |v| <= 2^17, and -inf -- class (NaN, +-0, +-inf) as torch's fp32 function stores it,
    finite results within 1 ulp of the float64 function rounded once"""
    from yolort_amd._lib import ACT_HARDSWISH, ACT_LEAKY, dtype_code
    pre = torch.cat([_exact.act_domain(dtype), torch.full((32,), float("-inf"), dtype=dtype)])
    buf = pre.clone().view(-1, 32)
    _check(sim, sim.ymi_act(buf.data_ptr(), 32, buf.shape[0], 32, dtype_code(dtype), ACT_HARDSWISH if act_name == "hardswish" else ACT_LEAKY, None, 0, None))
    worst, mean, cnt = _exact.assert_act_domain(buf.reshape(-1), pre.double(), act_name, dtype, 1, f"ymi_act {act_name} {dtype}")
    print(f"EXACT sim ymi_act {act_name} {str(dtype)[6:]}: worst {worst:.3f} ulp, mean signed {mean:+.4f} ulp over {cnt} values")
    assert abs(mean) <= 0.1


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_exact_silu_domain_through_a_pointwise_convolution(sim, dtype):
    """every finite fp16 value (bf16: |v| <= 2^17) as the pre-activation of the shared 16-bit epilogue, through an identity 1x1 convolution (tile 121, one launch): both ends
    of SiLU (exp2 overflowing to inf at v < -88.7: rcp(inf) = 0, the result is -0; underflowing at v > 88.7), subnormal results, +-0"""
    from yolort_amd import engine
    x, wt, bias, pre = _exact.silu_domain_problem(dtype)
    npix = x.shape[0]
    xb = Buf(1, 1, npix, 32, dtype, fill=x)
    yb = Buf(1, 1, npix, 64, dtype)
    pc = engine.PackedConv(wt.float().view(64, 32, 1, 1), bias.float(), None, dtype, torch.device("cpu"))
    _check(sim, sim.sim_conv2d(C.byref(_conv_desc(xb, pc, yb, 121))))
    got = yb.view().reshape(-1)
    worst, mean, cnt = _exact.assert_act_domain(got, pre.reshape(-1), "silu", dtype, 1, f"silu domain {dtype}")
    print(f"EXACT sim silu domain {str(dtype)[6:]}: worst {worst:.3f} ulp, mean signed {mean:+.4f} ulp over {cnt} values")
    assert abs(mean) <= 0.1
    if dtype == torch.float16:
        assert int(((got.float().abs() > 0) & (got.float().abs() < 2.0 ** -14)).sum()) > 1000   # subnormal results are part of the domain


# ---- the first layer on exact operands (tests/_stem_cases.py): the CPU half of tests/test_stem_exact_gpu.py ----------------------------------------------------------------
import _stem_cases as _stem  # noqa: E402

_STEM_SIM_SHAPES = _stem.SHAPES[:6]          # up to (3, 18, 72); fp16 adds one of the two larger maps
# (dtype, tile, shape, cout, weight set): the stem kernel (tile 41; the planar kernel runs the planar-capable ones of these too) at every cout on every shape, and generic
# tiles of the simulator build on the im2col-table form at one cout per shape (the 8-wave and row-transposed tiles need cin % 32 == 0 and refuse the form: the GPU half
# asserts that refusal for every id); ONE weight set per (shape, cout), rotating
_STEM_SIM = []
for _dt, _tiles, _shapes, _k in ((torch.float16, [41, 12, 24], _STEM_SIM_SHAPES + [_stem.SHAPES[6]], 0), (torch.bfloat16, [41, 21, 27], _STEM_SIM_SHAPES, 7)):
    for _j, _tile in enumerate(_tiles):
        for _i, _shape in enumerate(_shapes):
            for _c, _cout in enumerate(_stem.COUTS):
                if _tile == 41 or (_i + _j) % 4 == _c:
                    _STEM_SIM.append((_dt, _tile, _shape, _cout, (_i + _j + _k) % _stem.SETS[_cout]))
for _cout in _stem.COUTS:   # the single-tap channels of the stem-kernel launches reach all 108 taps at every cout
    assert _stem.tap_cover([(c, s) for (_, t, _, c, s) in _STEM_SIM if c == _cout and t == 41]) == set(range(_stem.NTAPS)), _cout


def _stem_sim_desc(cv, pc, og, act, tile, dtype):
    """the stem's descriptor in its super-pixel form over a guarded canvas `cv` and output `og` (tests/_stem_cases.py Guard)"""
    from yolort_amd._lib import ACT_NONE, ACT_SILU, ConvDesc, dtype_code
    d = ConvDesc()
    d.x, d.w, d.bias, d.y = cv.ptr, pc.w.data_ptr(), pc.bias.data_ptr(), og.ptr
    d.n, d.h, d.w_in, d.cin, d.x_cstride = cv.n, cv.h, cv.w // 2, 8, 8
    d.ho, d.wo, d.cout, d.cout_pad, d.y_cstride = og.h, og.w, pc.cout, pc.cout_pad, og.cs
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.k_pad = 6, 3, 2, 1, 2, 1, pc.k_pad
    d.act, d.dtype, d.out_dtype, d.tile = ACT_SILU if act else ACT_NONE, dtype_code(dtype), dtype_code(og.t.dtype), tile
    d.zeros = cv.zeros
    kt = pc.ktab(cv.w // 2, 8)
    d.ktab = kt.data_ptr()
    d._keep = kt
    return d


def _stem_sim_out(n, ho, wo, cout, dtype, dense=False):
    cpu = torch.device("cpu")
    if dense:
        return _stem.Guard(n, ho, wo, cout, dtype, cpu).snapshot()
    return _stem.Guard(n, ho, wo, cout, dtype, cpu, c0=16, cs=(cout + 7) // 8 * 8 + 32).snapshot()


def _stem_sim_launch(sim, dtype, tile, x, pc, act, planar=False, out_dtype=None):
    """one stem launch from the guarded canvas (sim_conv2d) or the guarded planar images (sim_conv_stem_planar; the canvas is then all NaN) -> output or None (refused, nothing written)"""
    cpu = torch.device("cpu")
    n, _, h, w = x.shape
    ho, wo = _stem.stem_hw(h, w)
    og = _stem_sim_out(n, ho, wo, pc.cout, out_dtype or dtype)
    label = f"stem {'planar' if planar else 'canvas'} tile {tile} {dtype} {(n, h, w)} cout {pc.cout}"
    if planar:
        cv = _stem.Guard(n, h, w, 4, dtype, cpu).snapshot()
        imgs, store = _stem.planar_images(x, dtype, cpu)
        before = store.clone()
        rc = sim.sim_conv_stem_planar(C.byref(_stem_sim_desc(cv, pc, og, act, 41, dtype)), (C.c_void_p * n)(*[im.data_ptr() for im in imgs]), n)
        assert torch.equal(_stem.bits(store), _stem.bits(before))
    else:
        cv = _stem.canvas(x, dtype, cpu)
        rc = sim.sim_conv2d(C.byref(_stem_sim_desc(cv, pc, og, act, tile, dtype)))
    cv.assert_untouched(label)
    if rc != 0:
        assert rc == -1, f"{label}: refusals carry YMI_EINVAL, got {rc}: {sim.sim_last_error().decode()}"
        og.assert_untouched(label + " (refused)")
        return None
    og.assert_only_the_view_written(label)
    return og.view().clone()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_exact_stem_per_element(sim, dtype):
    """conv_stem_kernel (tile 41), conv_stem_planar_kernel and generic tiles on the stem's im2col form, on exact operands inside NaN guard bands: no activation bit-identical to
    the once-rounded float64 reference (16-bit and, for the stem kernels, fp32 output), SiLU within 1 ulp and |mean| <= 0.1 ulp; planar == canvas bit for bit; W % 8 != 0 is
    refused by the planar entry point; tile 41 must never refuse"""
    from yolort_amd import engine
    cpu = torch.device("cpu")
    tally = {0: _exact.Tally(), 1: _exact.Tally(), "f32": _exact.Tally()}
    ran, refused = {}, {}
    for (dt, tile, shape, cout, seed) in _STEM_SIM:
        if dt != dtype:
            continue
        x, wt, bias = _stem.stem_operands(*shape, cout, seed)
        pc = engine.PackedConv(wt.float(), bias.float(), None, dtype, cpu, stem_superpixel=True)
        small = _stem.group_of(shape) == "small maps"
        modes = ((0, 1, "f32") if tile == 41 else (0, 1)) if small else ((seed + cout // 16) % 2,)
        for mode in modes:
            act, odt = mode == 1, (torch.float32 if mode == "f32" else dtype)
            label = f"sim stem tile {tile} {dtype} {shape} cout {cout} set {seed} mode {mode}"
            got = _stem_sim_launch(sim, dtype, tile, x, pc, act, out_dtype=odt)
            if got is None:
                assert tile != 41, label
                tally[mode].refused += 1
                refused.setdefault(tile, []).append((shape, cout))
                continue
            ran[tile] = ran.get(tile, 0) + 1
            tally[mode].check(got, _stem.stem_reference64(*shape, cout, seed, act), odt, 1 if act else 0, label, group=_stem.group_of(shape))
            if tile == 41:
                twin = _stem_sim_launch(sim, dtype, 41, x, pc, act, planar=True, out_dtype=odt)
                if _stem.planar_ok(shape):
                    assert twin is not None and torch.equal(_stem.bits(twin), _stem.bits(got)), f"{label}: the planar form differs from the canvas form"
                else:
                    assert twin is None, f"{label}: the planar entry point took W % 8 != 0"
    print(f"STEM sim {dtype}: launches that ran per tile {ran}; refused {refused}")
    assert all(ran.get(t, 0) > 0 for (dt, t, _, _, _) in _STEM_SIM if dt == dtype), "a tile of the list refused every case"
    for mode in tally:
        tally[mode].verdict(f"sim stem {dtype} mode {mode}")


def _exact_focus(version, cout, wt, bias):
    from yolort_amd.v5.models.common import Focus
    m = Focus(3, cout, k=3, version=version).eval()
    bn = m.conv.bn
    with torch.no_grad():
        m.conv.conv.weight.copy_(wt.float())
        bn.weight.copy_(torch.sqrt(bn.running_var.detach().to(torch.float32) + float(bn.eps)))   # as PackedConv computes it: scale = gamma / gamma = 1.0
        bn.running_mean.zero_()
        bn.bias.copy_(bias.float())
    return m


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("version", ["r4.0", "r3.1"])
def test_exact_focus_against_the_reference_formulation(sim, version, dtype):
    """Focus(3, 32, k=3) through Focus.packed() (stem_weight's rearrangement, the exact BatchNorm fold) and the stem kernel, against Conv(12, 32, 3, 1, 1) over
    focus_transform(x) in float64 -- the reference formulation: no activation bit-identical; SiLU (r4.0) 1 ulp; Hardswish (r3.1, its own ymi_act launch) 1 ulp"""
    from yolort_amd._lib import ACT_HARDSWISH, dtype_code
    cpu, cout = torch.device("cpu"), 32
    tally = {"none": _exact.Tally(), "act": _exact.Tally()}
    shapes = [s for s in _STEM_SIM_SHAPES if s[1] % 2 == 0]
    for i, shape in enumerate(shapes):
        seed = i % _stem.SETS[cout]
        x, wt, bias = _stem.focus_operands(*shape, cout, seed)
        pre = _stem.focus_pre64(*shape, cout, seed)
        pc = _exact_focus(version, cout, wt, bias).packed(dtype, cpu)
        w6 = pc.w[:cout, :144].float().view(cout, 6, 3, 2, 4)
        assert float(w6[..., 3].abs().max()) == 0 and torch.equal(pc.bias[:cout].double(), bias)
        assert torch.equal(F.conv2d(x, w6[..., :3].reshape(cout, 6, 6, 3).permute(0, 3, 1, 2).double(), bias, 2, 2), pre), "the packed weights do not carry the intended bits"
        p = pre.permute(0, 2, 3, 1).contiguous()
        for which in ("none", "act"):
            label = f"sim focus {version} {dtype} {shape} set {seed} {which}"
            got = _stem_sim_launch(sim, dtype, 41, x, pc, which == "act" and version == "r4.0")
            assert got is not None, label
            if which == "none":
                ref = p
            elif version == "r4.0":
                ref = _exact.silu64(p)
            else:
                buf = got.contiguous()
                _check(sim, sim.ymi_act(buf.data_ptr(), cout, buf.numel() // cout, cout, dtype_code(dtype), ACT_HARDSWISH, None, 0, None))
                got, ref = buf, _exact.ACT_REFS["hardswish"][0](_exact.round_once(p, dtype).double())
            tally[which].check(got, ref, dtype, 0 if which == "none" else 1, label, group=_stem.group_of(shape))
    assert _stem.tap_cover([(cout, i % _stem.SETS[cout]) for i in range(len(shapes))]) == set(range(_stem.NTAPS))
    for which in tally:
        tally[which].verdict(f"sim focus {version} {dtype} {which}")


def _stem_sim_fused(sim, dtype, x, w0, b0, w1, b1, form, label):
    """body.1's output of the ONE launch (planar images / canvas) and of the two launches (the form's stem kernel, then tile 131), guard bands asserted -> (fused, separate)"""
    from yolort_amd import engine
    cpu = torch.device("cpu")
    n, _, h, w = x.shape
    hs, ws = _stem.stem_hw(h, w)
    ho, wo = _stem.body1_hw(hs, ws)
    pc0 = engine.PackedConv(w0.float(), b0.float(), None, dtype, cpu, stem_superpixel=True)
    pc1 = engine.PackedConv(w1.float(), b1.float(), None, dtype, cpu)
    kt = pc1.ktab(ws, 32)
    outs = {}
    for fused in (False, True):
        cv = _stem.canvas(x, dtype, cpu) if form == "canvas" else _stem.Guard(n, h, w, 4, dtype, cpu).snapshot()
        sg, og = _stem_sim_out(n, hs, ws, 32, dtype, dense=True), _stem_sim_out(n, ho, wo, 64, dtype)
        d0 = _stem_sim_desc(cv, pc0, sg, True, 41, dtype)
        d1 = _conv_desc(sg, pc1, og, 131, k=3, pad=1, stride=2)
        d1.ktab = kt.data_ptr()
        imgs, store = _stem.planar_images(x, dtype, cpu) if form == "planar" else ([], None)
        ptrs = (C.c_void_p * n)(*[im.data_ptr() for im in imgs]) if form == "planar" else None
        if fused:
            _check(sim, sim.sim_stem_body1_planar(C.byref(d0), C.byref(d1), ptrs, n) if form == "planar" else sim.sim_stem_body1(C.byref(d0), C.byref(d1)))
            sg.assert_untouched(f"{label}: the stem's output buffer")
        else:
            _check(sim, sim.sim_conv_stem_planar(C.byref(d0), ptrs, n) if form == "planar" else sim.sim_conv2d(C.byref(d0)))
            sg.assert_only_the_view_written(f"{label}: the stem's output")
            _check(sim, sim.sim_conv2d(C.byref(d1)))
        og.assert_only_the_view_written(f"{label} fused={fused}")
        cv.assert_untouched(label)
        outs[fused] = og.view().clone()
    return outs[True], outs[False]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("form", ["planar", "canvas"])
def test_exact_fused_stem_body1(sim, form, dtype):
    """stem + body.1 as one launch on exact operands, both input forms: bit-identical to the two launches (stem's output buffer untouched, NaN guard bands intact), and -- on
    the problem whose intermediate is exact (stem pre-activations are integers in [19, 61]; body.1 pads with 0, not 40) -- within 1 ulp of the independent float64 two-layer
    reference, |mean| <= 0.1 ulp, for the one launch and for the two"""
    w1, b1 = _stem.body1_weights()
    tally = {"fused": _exact.Tally(), "two launches": _exact.Tally()}
    shapes = _STEM_SIM_SHAPES + ([_stem.SHAPES[7]] if dtype == torch.float16 else [])
    for i, shape in enumerate(s for s in shapes if form == "canvas" or _stem.planar_ok(s)):
        seed = i % _stem.SETS[32]
        x, wt, bias = _stem.stem_operands(*shape, 32, seed)
        label = f"sim fused {form} {dtype} {shape} set {seed}"
        one, two = _stem_sim_fused(sim, dtype, x, wt, bias, w1, b1, form, label)
        assert torch.equal(_stem.bits(one), _stem.bits(two)), f"{label}: differs from the two launches"
        x, w0, b0, w1x, b1x = _stem.two_layer_operands(*shape)
        label = f"sim two-layer {form} {dtype} {shape}"
        one, two = _stem_sim_fused(sim, dtype, x, w0, b0, w1x, b1x, form, label)
        ref = _stem.two_layer_reference64(*shape)
        tally["fused"].check(one, ref, dtype, 1, label + " fused", group=_stem.group_of(shape))
        tally["two launches"].check(two, ref, dtype, 1, label + " two launches", group=_stem.group_of(shape))
    for k in tally:
        tally[k].verdict(f"sim fused stem + body.1 {form} {dtype} {k}")
