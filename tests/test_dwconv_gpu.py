"""The depthwise kernel (ymi_dwconv2d, csrc/dwconv.hip) on the MI355X, driven through ctypes on poisoned outputs, and the blocks built on it.

Operands follow tests/_exact.py's recipe: activations are integers in [-3, 3], weights integers in [-2, 2] / 8, the bias a multiple of 1/8 (every fourth one large),
the shortcut a multiple of 1/4.  A 25-tap sum is then a multiple of 1/8 below 25 * 3/4 + 4096 + 8 < 2^13: exact in fp32 in any order, so the float64 value of
F.conv2d(groups=c) + bias (+ shortcut), rounded once to the storage type, is the one right answer.  Channel o < k * k carries ONE non-zero weight, at tap o."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import _exact
import _ghost

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
POISON, GUARD = 123.0, 64
KINDS = [(3, 1), (3, 2), (5, 1), (5, 2)]


@pytest.fixture(scope="module")
def dev():
    from yolort_amd import _lib
    _lib.load(require_gpu=True)
    return torch.device("cuda:0")


def shapes(s):
    """(n, h, w, c): one-pixel / one-row / one-column maps, a map smaller than the 5 x 5 window with a partial second slab, ragged maps, several partial tiles, and the map
    whose output exceeds one workgroup tile by exactly one pixel both ways at stride s"""
    from yolort_amd._lib import DWCONV_TILE
    th, tw = DWCONV_TILE[s]
    return [(1, 1, 1, 8), (1, 1, 7, 8), (1, 7, 1, 16), (2, 3, 3, 72), (3, 5, 4, 64), (1, 17, 33, 136), (1, th * s + 1, tw * s + 1, 72)]


@functools.lru_cache(maxsize=None)
def operands(n, h, w, c, k, s):
    """x (n, c, h, w), weight (c, 1, k, k), bias (c), shortcut (n, ho, wo, c) in float64, and the float64 pre-activation in NHWC (shared: do not modify)"""
    g = torch.Generator().manual_seed(97 * c + 7 * h + 3 * w + k + s)
    ho, wo = _exact.out_hw(h, w, k, s)
    x = torch.randint(-_exact.A_MAX, _exact.A_MAX + 1, (n, c, h, w), generator=g).double()
    q = torch.randint(-_exact.W_MAX, _exact.W_MAX + 1, (c, 1, k, k), generator=g)
    for o in range(min(k * k, c - 2)):
        q[o] = 0
        q[o, 0, o // k, o % k] = (1, -2, 2)[o % 3]
    wt = q.double() / _exact.W_DEN
    bias = torch.randint(-16, 17, (c,), generator=g).double() / 8
    bias[3::4] = torch.tensor([1000.125, -2049.625, 33.125, -515.625, 4095.875, -1027.375], dtype=torch.float64)[torch.arange(len(bias[3::4])) % 6]
    res = torch.randint(-32, 33, (n, ho, wo, c), generator=g).double() / 4
    pre = F.conv2d(x, wt, bias, s, k // 2, groups=c).permute(0, 2, 3, 1).contiguous()
    assert not bool(((pre < -80) & (pre > -300)).any())      # (the band where fp32 SiLU underflows: _exact.reference64)
    return x, wt, bias, res, pre


def _view(dev, dtype, data, shape, off):
    """a POISON-filled flat buffer [guard | (n, h, w, cs) | guard] holding `data` (NHWC) from channel `off` on -> (buffer, element offset, pixel stride, strides)"""
    n, h, w, c = shape
    cs = c + 24 if off else c
    buf = torch.full((2 * GUARD + n * h * w * cs,), POISON, dtype=dtype, device=dev)
    st = (h * w * cs, w * cs, cs, 1)
    if data is not None:
        torch.as_strided(buf, shape, st, GUARD + off).copy_(data.to(dtype))
    return buf, GUARD + off, cs, st


def launch(dev, dtype, case, k, s, act=0, residual=False, strided=False):
    """one ymi_dwconv2d call on exact operands -> the (n, ho, wo, c) output on the CPU.  strided: x and res are channels [8, 8 + c) of c + 24, y channels [16, 16 + c);
    everything of y's buffer outside the view -- guard bands, the other channels -- must still hold POISON"""
    from yolort_amd import _lib
    n, h, w, c = case
    x, wt, bias, res, _ = operands(n, h, w, c, k, s)
    oshape = (n, *_exact.out_hw(h, w, k, s), c)
    xb, xo, xcs, _ = _view(dev, dtype, x.permute(0, 2, 3, 1), (n, h, w, c), 8 * strided)
    rb, ro, rcs, _ = _view(dev, dtype, res, oshape, 8 * strided)
    yb, yo, ycs, yst = _view(dev, dtype, None, oshape, 16 * strided)
    wp, bp = wt.reshape(c, k * k).t().contiguous().to(dtype).to(dev), bias.float().to(dev)
    d = _lib.DwConvDesc(x=xb.data_ptr() + 2 * xo, w=wp.data_ptr(), bias=bp.data_ptr(), y=yb.data_ptr() + 2 * yo, res=rb.data_ptr() + 2 * ro if residual else None,
                        n=n, h=h, w_in=w, c=c, x_cstride=xcs, y_cstride=ycs, res_cstride=rcs if residual else 0, ho=oshape[1], wo=oshape[2], k=k, s=s, p=k // 2, act=act,
                        dtype=_lib.dtype_code(dtype))
    _lib.check(_lib.load().ymi_dwconv2d(C.byref(d), _lib.stream_ptr()), "ymi_dwconv2d")
    torch.cuda.synchronize()
    full = yb.cpu()
    got = torch.as_strided(full, oshape, yst, yo).clone()
    torch.as_strided(full, oshape, yst, yo).fill_(POISON)
    assert bool((full == POISON).all()), f"{case} k{k} s{s}: a write outside the output view"
    return got


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("k,s", KINDS)
def test_exact_operands_bit_for_bit(dev, k, s, dtype, residual):
    """act = none: the once-rounded float64 value, bit for bit, contiguous and as channel slices of wider poisoned buffers"""
    for case in shapes(s):
        _, _, _, res, pre = operands(*case, k, s)
        want = _exact.round_once(pre + res if residual else pre, dtype)
        for strided in (False, True):
            got = launch(dev, dtype, case, k, s, 0, residual, strided)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{case} k{k} s{s} strided={strided}: {int((got != want).sum())} elements differ"


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("act_name,act", [("silu", 1), ("hardswish", 2), ("leaky", 3)])
def test_activations(dev, act_name, act, dtype):
    """the float64 activation of the exact pre-activation (+ shortcut): SiLU by _exact's criterion (1 ulp, mean signed error within 0.1 ulp), Hardswish / LeakyReLU bit for bit"""
    tally = _exact.Tally()
    for k, s in KINDS:
        for i, case in enumerate(shapes(s)):
            _, _, _, res, pre = operands(*case, k, s)
            ref = _exact.ACT_REFS[act_name][0](pre)      # (Hardswish of v <= -3 is -0.0, in float64 as in the kernel: nothing is added where there is no shortcut)
            got = launch(dev, dtype, case, k, s, act, bool(i % 2))
            tally.check(got, ref + res if i % 2 else ref, dtype, 1 if act == 1 else 0, f"{act_name} {case} k{k} s{s}", group="large map" if i == 5 else "small maps")
    tally.verdict(f"gpu dwconv {act_name} {str(dtype)[6:]}")


@pytest.mark.parametrize("name", sorted(_ghost.CASES))
def test_blocks_against_float64_torch(dev, name):
    m, twin = _ghost.pair(name)
    g = torch.Generator().manual_seed(100)
    with torch.no_grad():
        for mod in m.modules():      # non-trivial BatchNorm statistics, as tests/_blocks.build sets them
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) * 0.8 + 0.6)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.2)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
        x = torch.randn((1, 64, 16, 16), generator=g)
        twin.load_state_dict(m.state_dict())
        want = twin.double()(x.double())
    m = m.to(dev).half()
    out = m(x.to(dev).half())
    assert tuple(out.shape) == tuple(want.shape) and out.dtype == F16
    assert (out.double().cpu() - want).abs().max().item() <= 1e-2 * max(1.0, want.abs().max().item()), name
    assert torch.equal(out, m(x.to(dev).half()))      # the cached plan replays


def test_graph_capture_replays_bit_for_bit(dev, tmp_path):
    """a plan holding the op (a GhostConv: 1x1, then the depthwise 5x5 on a channel slice), captured: replays on changed input equal the per-kernel launches"""
    from yolort_amd import engine
    from yolort_amd.v5 import GhostConv
    torch.manual_seed(3)
    plan = engine.Plan(dev, F16)
    xv = plan.alloc(2, 9, 21, 32)
    out = GhostConv(32, 64).eval().emit(plan, xv)
    stream = torch.cuda.Stream()
    for i in range(3):
        xv.as_tensor().copy_(torch.randn(2, 9, 21, 32, generator=torch.Generator().manual_seed(i)).half())
        plan.run()
        torch.cuda.synchronize()
        eager = out.as_tensor().clone()
        out.as_tensor().zero_()
        torch.cuda.synchronize()
        plan.run(graph=True, stream=stream)
        torch.cuda.synchronize()
        assert bool(eager.abs().sum() > 0) and torch.equal(out.as_tensor(), eager), i
    assert all(ms >= 0 for _, ms, _ in plan.profile(1)) and [meta["kind"] for meta in plan.meta] == ["conv", "dwconv"]
    # an exported plan carries the op: imported into fresh device memory through the C ABI alone, it replays to the same output
    from yolort_amd._lib import PlanRegion, TAG_BOXES, TAG_INPUT
    path = str(tmp_path / "ghost.ymiplan")
    plan.export(path, io={TAG_INPUT: xv.base, TAG_BOXES: out.base})
    plan2, regs, nreg = C.c_void_p(), (PlanRegion * 64)(), C.c_int(0)
    assert plan.lib.ymi_plan_import(path.encode(), C.byref(plan2), regs, 64, C.byref(nreg)) == 0, plan.lib.ymi_last_error()
    by_tag = {regs[i].tag: regs[i] for i in range(nreg.value) if regs[i].tag}
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    got = torch.zeros_like(out.base)
    try:
        assert hip.hipMemcpy(by_tag[TAG_INPUT].base, xv.base.data_ptr(), xv.base.numel() * 2, 3) == 0
        assert plan.lib.ymi_plan_run(plan2, 0, -1, 0, C.c_void_p(stream.cuda_stream)) == 0, plan.lib.ymi_last_error()
        stream.synchronize()
        assert hip.hipMemcpy(got.data_ptr(), by_tag[TAG_BOXES].base, got.numel() * 2, 3) == 0
        torch.cuda.synchronize()
    finally:
        plan.lib.ymi_plan_destroy(plan2)
    assert torch.equal(got, out.base)
