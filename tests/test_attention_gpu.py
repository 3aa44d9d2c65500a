"""The attention kernel (ymi_attention, csrc/attention.hip) on the MI355X against the float64 soft-max attention, and the transformer blocks built on it.  Every launch
reads q / k / v as channels [0, c), [c, 2c), [2c, 3c) of one poisoned (3c + 24)-channel buffer and writes channels [16, 16 + c) of a poisoned (c + 24)-channel buffer
between guard bands; everything outside the output view must still hold the poison."""
import ctypes as C

import pytest
import torch

import _attn_cases as A
import _exact

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
POISON, GUARD = 123.0, 64


@pytest.fixture(scope="module")
def dev():
    from yolort_amd import _lib
    _lib.load(require_gpu=True)
    return torch.device("cuda:0")


def launch(dev, dtype, kind, case):
    """one ymi_attention call on the operands of `kind` -> (output (n, S, c) on the CPU, q, k, v in float64, the picked keys)"""
    from yolort_amd import _lib
    n, h, w, heads, d = case
    s, c = h * w, heads * d
    q, k, v, perm = A.operands(kind, n, s, heads, d)
    ics, ocs = 3 * c + 24, c + 24
    ib = torch.full((2 * GUARD + n * s * ics,), POISON, dtype=dtype, device=dev)
    ob = torch.full((2 * GUARD + n * s * ocs,), POISON, dtype=dtype, device=dev)
    torch.as_strided(ib, (n, s, 3 * c), (s * ics, ics, 1), GUARD).copy_(torch.cat([q, k, v], 2).to(dtype))
    desc = _lib.AttnDesc(q=ib.data_ptr() + 2 * GUARD, k=ib.data_ptr() + 2 * (GUARD + c), v=ib.data_ptr() + 2 * (GUARD + 2 * c), o=ob.data_ptr() + 2 * (GUARD + 16), n=n, S=s,
                         heads=heads, d=d, c=c, q_cstride=ics, k_cstride=ics, v_cstride=ics, o_cstride=ocs, dtype=_lib.dtype_code(dtype), scale=d ** -0.5)
    _lib.check(_lib.load().ymi_attention(C.byref(desc), _lib.stream_ptr()), "ymi_attention")
    torch.cuda.synchronize()
    full = ob.cpu()
    view = torch.as_strided(full, (n, s, c), (s * ocs, ocs, 1), GUARD + 16)
    got = view.clone()
    view.fill_(POISON)
    assert bool((full == POISON).all()), f"{case}: a write outside the output view"
    return got, q, k, v, perm


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("case", A.shapes())
def test_selection_bit_for_bit(dev, case, dtype):
    """the picked key leads every other by 512 / sqrt(d) >= 45 after scaling: the output IS row perm(i) of v, in both dtypes"""
    got, _, _, v, perm = launch(dev, dtype, "select", case)
    n, s, heads, d = case[0], case[1] * case[2], case[3], case[4]
    want = torch.gather(v.reshape(n, s, heads, d), 1, perm[..., None].expand(n, s, heads, d)).reshape(n, s, -1)
    _exact.assert_elementwise(got, want, dtype, 0, f"select {case}")


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("case", A.shapes())
def test_uniform_weights_give_the_column_mean(dev, case, dtype):
    """q = 0: every key < S weighs 1 / S and nothing else weighs anything -- the once-rounded float64 column mean of v, to 1 ulp"""
    got, _, _, v, _ = launch(dev, dtype, "uniform", case)
    _exact.assert_elementwise(got, v.mean(1, keepdim=True).expand_as(v), dtype, 1, f"uniform {case}")


@pytest.mark.parametrize("dtype,u", [(F16, 2.0 ** -11), (BF16, 2.0 ** -8)])
def test_general_values_within_the_derived_bound(dev, dtype, u):
    """|got - ref| <= 3 u max_j |v[n, j, h, ch]| + u |ref| per element: the weights are rounded to the storage type before P V (u max|v|; 2 u had the row sum been taken
    from the rounded weights), the final rounding adds u / 2 |ref|; the fp32 effects are orders of magnitude below.  Largest observed fraction of the bound on the
    MI355X: see profiles/attention_bench.txt."""
    worst = 0.0
    for case in A.shapes():
        got, q, k, v, _ = launch(dev, dtype, "general", case)
        ref = A.reference64(q, k, v, case[3], case[4] ** -0.5)
        frac = ((got.double() - ref).abs() / (3 * u * v.abs().amax(1, keepdim=True) + u * ref.abs())).nan_to_num(0.0).max().item()      # (0 / 0: an exact zero)
        print(f"ATTN general {str(dtype)[6:]} {case}: {frac:.3f} of the bound")
        worst = max(worst, frac)
    assert worst <= 1.0, worst


def test_ops_attention_reads_slices_in_place(dev):
    """the stand-alone op on three channel slices of one (n, H, W, 3c) tensor equals the direct launch bit for bit and keeps the input's shape"""
    from yolort_amd import ops
    case = (1, 10, 15, 4, 64)
    got, q, k, v, _ = launch(dev, BF16, "general", case)
    qkv = torch.cat([q, k, v], 2).reshape(1, 10, 15, 768).to(BF16).to(dev)
    out = ops.attention(qkv[..., :256], qkv[..., 256:512], qkv[..., 512:], 4)
    assert out.shape == (1, 10, 15, 256) and torch.equal(out.cpu().reshape(1, 150, 256), got)


def _randomise(m, g):
    """non-trivial BatchNorm statistics and biases (nn.MultiheadAttention's start at zero)"""
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) * 0.8 + 0.6)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_blocks_against_float64_torch(dev, name):
    """the float64 evaluation of the UNFOLDED nn twin, by the block-level criterion of tests/test_dwconv_gpu.py; the second run replays the cached plan bit for bit"""
    m, twin = A.pair(name)
    g = torch.Generator().manual_seed(100)
    _randomise(m, g)
    x = torch.randn((2, A.CASES[name][0], 6, 5), generator=g)
    twin.load_state_dict(m.state_dict())
    with torch.no_grad():
        x64 = x.double()
        want = twin.double()(x64.flatten(2).permute(2, 0, 1)).permute(1, 2, 0).reshape(x.shape) if name == "TransformerLayer" else twin.double()(x64)
    m = m.to(dev).half()
    out = m(x.to(dev).half())
    assert tuple(out.shape) == tuple(want.shape) and out.dtype == F16
    assert (out.double().cpu() - want).abs().max().item() <= 1e-2 * max(1.0, want.abs().max().item()), name
    assert torch.equal(out, m(x.to(dev).half()))


def test_graph_capture_and_exported_plan_replay_bit_for_bit(dev, tmp_path):
    """a C3TR plan: captured replays on changed input equal the per-kernel launches; exported and imported through the C ABI alone it replays to the same output"""
    from yolort_amd import engine
    from yolort_amd._lib import PlanRegion, TAG_BOXES, TAG_INPUT
    m, _ = A.pair("C3TR")
    _randomise(m, torch.Generator().manual_seed(3))
    plan = engine.Plan(dev, F16)
    xv = plan.alloc(2, 9, 8, 64)
    out = m.to(dev).half().emit(plan, xv)
    stream = torch.cuda.Stream()
    for i in range(3):
        xv.as_tensor().copy_(torch.randn(2, 9, 8, 64, generator=torch.Generator().manual_seed(i)).half())
        plan.run()
        torch.cuda.synchronize()
        eager = out.as_tensor().clone()
        out.as_tensor().zero_()
        torch.cuda.synchronize()
        plan.run(graph=True, stream=stream)
        torch.cuda.synchronize()
        assert bool(eager.abs().sum() > 0) and torch.equal(out.as_tensor(), eager), i
    assert all(ms >= 0 for _, ms, _ in plan.profile(1)) and [meta["kind"] for meta in plan.meta] == ["conv", "conv", "conv", "attention", "conv", "conv", "conv"]
    path = str(tmp_path / "c3tr.ymiplan")
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
