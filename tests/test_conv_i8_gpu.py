"""The int8 convolution and the quantise kernel on the device (csrc/conv_i8.hip) against a yardstick that shares nothing with them: torch's float64 conv2d on the
integer codes (exact: every partial sum is an integer below 2^53) and a float64 epilogue (_i8_cases.reference).

THE BOUND.  The contract (include/yolort_amd.h) fixes the fp32 steps, so their error against float64 is bounded step by step, u = 2^-24:
  conversion  |float(acc) - acc| <= u |acc| (zero below 2^24)
  fma         pre32 = fl(f * scale + bias): |pre32 - pre| <= u |acc scale| + u |pre|                                   =: e_pre
  activation  identity: e_pre.  LeakyReLU: one multiplication by fp32(0.1), itself within u of 0.1: e_pre + 2 u |a|.  Hardswish: slope <= 1.5, an addition, a
              multiplication and a division: 1.5 e_pre + 4 u |a|.  SiLU: slope <= 1.1; the project's criterion for its hardware exp2 / rcp form is 1 ulp of the fp32
              value (2 u |a|, tests/_exact.py), to which the rounding of the exponent's argument (relative |pre| u in exp(-pre), at most that in a) and of the sum and
              the product (2 u each) are added: 1.1 e_pre + (6 + |pre|) u |a|
  shortcut    one fma: + u |post|                                                                                          =: e_post
  int8        code = post * fl(1 / out_scale): two roundings: e_post / out_scale + 2 u |code|                              =: delta
An int8 element must equal clamp(rint(code64)) unless code64 lies within delta of a half-integer, where it may differ by one code; at most 1 % of a case's elements may
be such (checked on the float64 reference alone).  A 16-bit element must lie within half a spacing of its type at the reference plus e_post.  Where the operands are
exact -- the "distinct" cases: power-of-two scale, integer bias, identity -- the 16-bit result is the once-rounded reference bit for bit.
"""
import ctypes as C

import pytest
import torch

import _i8_cases as cases
from _i8_cases import ACT_HARDSWISH, ACT_LEAKY, ACT_NONE, ACT_SILU

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _packed(wq, scale, bias):
    """PackedConvI8 of given codes and epilogue vectors (in_scale 1, w_scale = scale)"""
    from yolort_amd.engine import PackedConvI8
    return PackedConvI8.from_quantized(wq, scale.double(), bias, 1.0, torch.device(DEV))


def _run(case, act, out_scale, dtype=torch.float16, with_res=False, res_scale=1.0, seed=0):
    from yolort_amd import ops
    n, h, w, cin, cout, k, s, _ = case
    xq, wq, scale, bias = cases.operands(case, seed)
    pc = _packed(wq, scale, bias)
    res = None
    if with_res:
        ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
        g = torch.Generator().manual_seed(seed + 1)
        res = torch.randint(-127, 128, (n, cout, ho, wo), generator=g).to(torch.int8) if out_scale is not None else torch.randn(n, cout, ho, wo, generator=g).to(dtype)
    got = ops.conv2d_int8(xq.to(DEV), pc, s, act, out_scale, None if res is None else res.to(DEV), res_scale, dtype)
    post, err = cases.reference(xq, wq, pc.scale.cpu(), pc.bias.cpu(), k, s, act, res, res_scale)
    return got, post, err


@pytest.mark.parametrize("name", sorted(cases.CONV_CASES))
def test_int8_output_matches_the_integer_reference(name):
    case = cases.CONV_CASES[name]
    out_scale = {"distinct": 2.0, "extreme": 0.25}.get(case[7], 0.05)
    got, post, err = _run(case, ACT_NONE if case[7] != "random" else ACT_SILU, out_scale)
    cases.check_int8(got, post, err, out_scale)
    if case[7] == "extreme":   # the sums pass 2^24, and the output saturates at both ends
        assert float(post.abs().max()) > 2 ** 24 * 1e-6 and int(got.max()) == 127 and int(got.min()) == -127 and float((got.abs() == 127).float().mean()) >= 0.5


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", sorted(cases.CONV_CASES))
def test_16_bit_output_is_one_rounding_of_the_reference(name, dtype):
    case = cases.CONV_CASES[name]
    got, post, err = _run(case, ACT_NONE, None, dtype)
    cases.check_16(got, post, err, dtype)
    if case[7] == "distinct":
        assert torch.equal(got.cpu(), post.float().to(dtype)), "exact operands: the result must be the once-rounded reference bit for bit"


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("out", ["int8", torch.float16, torch.bfloat16])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_SILU, ACT_HARDSWISH, ACT_LEAKY])
def test_epilogue_variants(act, out, with_res):
    if out == "int8":
        got, post, err = _run(cases.EPILOGUE_SHAPE, act, 0.04, with_res=with_res, res_scale=0.032, seed=act)
        cases.check_int8(got, post, err, 0.04)
    else:
        got, post, err = _run(cases.EPILOGUE_SHAPE, act, None, out, with_res=with_res, seed=act)
        cases.check_16(got, post, err, out)


def test_channel_slice_views_leave_their_neighbours_untouched():
    """input, output and shortcut are channel slices of wider buffers (cstride > c) whose other bytes are poisoned"""
    from yolort_amd.engine import Plan
    case = (2, 9, 11, 32, 24, 3, 1, "random")
    n, h, w, cin, cout, k, s, _ = case
    xq, wq, scale, bias = cases.operands(case)
    res = torch.randint(-127, 128, (n, cout, h, w), generator=torch.Generator().manual_seed(5)).to(torch.int8)
    plan = Plan(torch.device(DEV), torch.float16)
    xb, yb, rb = plan.alloc(n, h, w, 64, torch.int8), plan.alloc(n, h, w, 48, torch.int8), plan.alloc(n, h, w, 40, torch.int8)
    for b in (xb, yb, rb):
        b.as_tensor().fill_(77)
    xv, yv, rv = xb.slice_c(16, cin), yb.slice_c(8, cout), rb.slice_c(16, cout)
    xv.as_tensor().copy_(xq.permute(0, 2, 3, 1))
    rv.as_tensor().copy_(res.permute(0, 2, 3, 1))
    plan.conv_i8(xv, _packed(wq, scale, bias), s, ACT_SILU, out_scale=0.05, out=yv, res=rv, res_scale=0.02)
    plan.run()
    torch.cuda.synchronize()
    post, err = cases.reference(xq, wq, scale, bias, k, s, ACT_SILU, res, 0.02)
    cases.check_int8(yv.as_tensor().permute(0, 3, 1, 2), post, err, 0.05)
    ya = yb.as_tensor()
    assert bool((ya[..., :8] == 77).all()) and bool((ya[..., 8 + cout:] == 77).all())
    assert torch.equal(xb.as_tensor()[..., 16:16 + cin].cpu(), xq.permute(0, 2, 3, 1)) and bool((xb.as_tensor()[..., :16] == 77).all()) and bool((rb.as_tensor()[..., :16] == 77).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("c,misaligned", [(32, False), (20, False), (32, True)])
def test_quantize_matches_rint_and_clip(dtype, c, misaligned):
    """power-of-two scale: exact ties go to even; NaN -> 0, +-inf -> +-127, values beyond +-127 steps clamp.  c = 32 takes the 16-byte form, c = 20 (no multiple of
    16) and a view that starts one channel into a wider buffer the scalar form"""
    from yolort_amd import _lib
    lib = _lib.load(require_gpu=True)
    scale, npix, cs = 0.25, 37, 48
    x = (torch.randint(-1200, 1200, (npix, cs), generator=torch.Generator().manual_seed(c)).double() * 0.125).to(dtype)   # multiples of scale / 2: every other one a tie
    x[0, :8] = torch.tensor([float("nan"), float("inf"), -float("inf"), 1000.0, -1000.0, 0.125, 0.375, -0.125], dtype=dtype)
    off = 1 if misaligned else 0
    xd = x.to(DEV)
    y = torch.full((npix, cs), 77, dtype=torch.int8, device=DEV)
    d = _lib.QuantI8Desc(x=xd.data_ptr() + off * xd.element_size(), y=y.data_ptr() + off, npix=npix, c=c - off, x_cstride=cs, y_cstride=cs, dtype=_lib.dtype_code(dtype), scale=scale)
    _lib.check(lib.ymi_quantize_i8(C.byref(d), _lib.stream_ptr()), "ymi_quantize_i8")
    want = cases.quantize_reference(x[:, off:c], scale)
    assert torch.equal(y[:, off:c].cpu(), want) and bool((y[:, :off] == 77).all()) and bool((y[:, c:] == 77).all())
    assert want[0, :8 - off].tolist() == [0, 127, -127, 127, -127, 0, 2, 0][off:]


def _chain(dtype=torch.float16):
    from yolort_amd.v5 import Conv, QConv
    torch.manual_seed(11)
    convs = [Conv(32, 32, 3, 1), Conv(32, 32, 1, 1)]
    for m in convs:
        m.bn.running_mean.normal_(0, 0.1)
        m.bn.running_var.uniform_(0.5, 1.5)
        m.bn.weight.data.uniform_(0.5, 1.5)
        m.bn.bias.data.normal_(0, 0.1)
    x = torch.randn(2, 32, 9, 11)
    in_scale, mid_scale = float(x.abs().max()) / 127, 4.0 / 127
    q1 = QConv.from_float(convs[0].eval(), in_scale, mid_scale).to(DEV)
    q2 = QConv.from_float(convs[1].eval(), mid_scale, None).to(DEV)
    return convs, q1, q2, x, in_scale, mid_scale


def test_plan_chain_replays_under_graph_capture_like_the_eager_ops():
    """quantize -> QConv (int8 out) -> QConv with a 16-bit shortcut (fp16 out), recorded once: eager and several graph replays equal the ops composition bit for bit"""
    from yolort_amd import ops
    from yolort_amd.engine import Plan
    from yolort_amd.hipmodule import nchw_to_view
    _, q1, q2, x, in_scale, _mid = _chain()
    xd = x.half().to(DEV)
    res = torch.randn(2, 32, 9, 11, generator=torch.Generator().manual_seed(2)).half().to(DEV)
    y1 = ops.conv2d_int8(ops.quantize_int8(xd, in_scale), q1.packed(torch.device(DEV)), 1, ACT_SILU, float(q1.out_scale))
    want = ops.conv2d_int8(y1, q2.packed(torch.device(DEV)), 1, ACT_SILU, None, res, 0.5, torch.float16)
    plan = Plan(torch.device(DEV), torch.float16)
    xin, rin = plan.alloc(2, 9, 11, 32, zero=True), plan.alloc(2, 9, 11, 32, zero=True)
    out = q2.emit(plan, q1.emit(plan, plan.quantize_i8(xin, in_scale)), res=rin, res_scale=0.5)
    assert plan.num_ops == 3 and out.dtype == torch.float16
    nchw_to_view(plan, xd, 32, out=xin)
    nchw_to_view(plan, res, 32, out=rin)
    stream = torch.cuda.Stream()
    for graph in (False, True, True, True):
        out.as_tensor().zero_()
        torch.cuda.synchronize()
        plan.run(graph=graph, stream=stream if graph else None)
        torch.cuda.synchronize()
        assert torch.equal(out.as_tensor().permute(0, 3, 1, 2), want), f"graph={graph}"


def test_qconv_from_float_against_its_conv_and_the_integer_reference():
    """|QConv - Conv| before the activation is bounded by half an input step times the L1 norm of the weight row plus half a weight step times the L1 norm of the
    quantised inputs under the window; SiLU's slope is at most 1.1, and the fp16 roundings of both outputs and the float Conv's own fp16 arithmetic (bounded by
    2^-10 of the L1 product) ride on top.  Against the integer reference the result is held to one rounding as everywhere."""
    convs, q1, _q2, x, in_scale, _ = _chain()
    from yolort_amd.v5 import QConv
    conv = convs[0].eval()
    q = QConv.from_float(conv, in_scale, None).to(DEV)
    xd = x.half().to(DEV)
    got = q(xd).double().cpu()
    ref_float = conv.half().to(DEV)(xd).double().cpu()
    pc = q.packed(torch.device(DEV))
    xh = x.half().double()
    xq = cases.quantize_reference(xh, in_scale)
    post, err = cases.reference(xq, pc.wq, pc.scale.cpu(), pc.bias.cpu(), 3, 1, ACT_SILU)
    cases.check_16(got, post, err, torch.float16)
    w64 = pc.wq.double() * pc.w_scale.view(-1, 1, 1, 1)
    l1_w = torch.nn.functional.conv2d(torch.ones_like(xh), w64.abs(), None, 1, 1)                      # L1 norm of the weight row under each window
    l1_x = torch.nn.functional.conv2d((xq.double() * in_scale).abs(), torch.ones_like(w64), None, 1, 1)   # L1 norm of the inputs under each window
    l1_xw = torch.nn.functional.conv2d(xh.abs(), w64.abs() + 0.5 * pc.w_scale.view(-1, 1, 1, 1), None, 1, 1)
    bound = 1.1 * (0.5 * in_scale * l1_w + 0.5 * pc.w_scale.view(1, -1, 1, 1) * l1_x + 2.0 ** -10 * l1_xw) + 2.0 ** -10 * (got.abs() + ref_float.abs()) + 1e-6
    assert bool(((got - ref_float).abs() <= bound).all()), float(((got - ref_float).abs() / bound).max())
