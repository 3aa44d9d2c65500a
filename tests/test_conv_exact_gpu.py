"""Per-element, rounding-level checks of every convolution kernel family on the GPU (helpers and the derivation of the operands: tests/_exact.py; the CPU half runs the
same families through the lane simulator, tests/test_hipsim_kernels.py).

The parity tests bound max|hip - ref| by 2e-3 / 1.6e-2 of the LARGEST output; a truncating 16-bit pack, a shortcut added after the rounding, a bias rounded to 16 bits or
a wrong tap at a border pixel whose output is small all fit inside.  Here the operands are exactly representable and the fp32 accumulation is exact in any order, so
  * without an activation every output must equal the float64 reference, rounded ONCE to the storage type, bit for bit (shortcut included);
  * with SiLU every output is within N ulp of the storage type and the mean signed error of a case is within 0.1 ulp (truncation shows as about -0.5).
N was not fixed in advance: v_exp_f32 and v_rcp_f32 are about 1 ulp of fp32 each, 2^-13 of an fp16 ulp, so the expectation is N = 1 (off by one only next to a rounding
tie), and that is what the parent commit measures on an MI355X -- see the docstrings of the tests for the figures per family.
Shapes: 1x1, 1xW and Hx1 maps (every tap but the centre is padding, a tile is almost entirely out of range), a map smaller than the window, ragged maps, several partial
tiles; 3x3 at strides 1 and 2; cin -> cout of 32 -> 32, 64 -> 128, 64 -> 40, 128 -> 64 and 48 -> 96 (the im2col-table form).  A family that does not take a shape
refuses it with YMI_EINVAL and writes nothing: that is asserted too.  Outputs are channel slices of wider buffers whose other channels must stay zero."""
import pytest
import torch

import _exact

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def dev():
    from yolort_amd import _lib
    _lib.load(require_gpu=True)
    return torch.device("cuda:0")


def _launch(dev, plan, dtype, tile, case, act, residual):
    """one launch through Plan.conv on exact operands -> (output (n, ho, wo, cout) on the CPU or None when the launch was refused with YMI_EINVAL, tile recorded in plan.meta)"""
    from yolort_amd import engine
    from yolort_amd._lib import ACT_NONE, ACT_SILU, YmiError
    n, h, w, cin, cout, k, s = case
    x, wt, bias, res = _exact.exact_operands(*case)
    ho, wo = _exact.out_hw(h, w, k, s)
    xv = plan.alloc(n, h, w, cin)
    xv.as_tensor().copy_(x.permute(0, 2, 3, 1).to(dtype).to(dev))
    pc = engine.PackedConv(wt.float(), bias.float(), None, dtype, dev)
    cpad = (cout + 7) // 8 * 8
    yb = plan.alloc(n, ho, wo, cpad + 32, zero=True)     # the output is a channel slice of a wider buffer
    yv = yb.slice_c(16, cout)
    rv = None
    if residual:
        rv = plan.alloc(n, ho, wo, cout)
        rv.as_tensor().copy_(res.permute(0, 2, 3, 1).to(dtype).to(dev))
    op = plan.num_ops
    plan.conv(xv, pc, s, k // 2, act=ACT_SILU if act else ACT_NONE, out=yv, res=rv, tile=tile)
    ran = plan.meta[op]["tile"]
    try:
        plan.run(op, op + 1)
    except YmiError as e:
        assert "(code -1)" in str(e), f"tile {tile} {case}: a refusal carries YMI_EINVAL: {e}"
        torch.cuda.synchronize()
        assert float(yb.as_tensor().float().abs().max()) == 0, f"tile {tile} {case}: refused, yet something was written"
        return None, ran
    torch.cuda.synchronize()
    full = yb.as_tensor().cpu()
    assert float(full[..., :16].float().abs().max()) == 0 and float(full[..., 16 + cout:].float().abs().max()) == 0, f"tile {tile} (ran {ran}) {case}: stray write outside the channel slice"
    return full[..., 16:16 + cout].contiguous(), ran


def _run_tile(dev, tile, dtype):
    from yolort_amd import engine
    plan = engine.Plan(dev, dtype)
    name = str(dtype)[6:]
    tally = {0: _exact.Tally(), 1: _exact.Tally()}
    substituted = {}
    for i, case in enumerate(_exact.cases(tile)):
        for act in (0, 1):
            residual = (i + act) % 2 == 0 and not (act and tile in _exact.NO_SHORTCUT)
            got, ran = _launch(dev, plan, dtype, tile, case, act, residual)
            if got is None and act == 0 and tile in _exact.SILU_ONLY:
                # a SiLU-only tile: what the library runs instead for an identity-activation launch of this shape is checked in its place
                got, ran = _launch(dev, plan, dtype, 0, case, act, residual)
                substituted[ran] = substituted.get(ran, 0) + 1
            if got is None:
                tally[act].refused += 1
                continue
            label = f"tile {tile} (ran {ran}) {name} {case} act={'silu' if act else 'none'} res={int(residual)}"
            # fp32 storage: SiLU + shortcut cancels, and the error of SiLU -- an ulp of ITS magnitude -- is many ulps of a small sum: the distance is measured at max(|SiLU|, |sum|)
            # -- and there the bound is N + 1 = 2: SiLU is off by at most N = 1 ulp of its own magnitude, the fp32 addition of the shortcut then rounds once more, and that
            # rounding and the reference's single one differ by at most one ulp of the sum
            scale = _exact.reference64(*case, True, False) if (dtype == F32 and act and residual) else None
            tally[act].check(got, _exact.reference64(*case, bool(act), residual), dtype, (2 if scale is not None else 1) if act else 0, label, group=_exact.group_of(case), scale64=scale)
    if substituted:
        print(f"EXACT tile {tile} {name} act=none: refused (SiLU only); the library's rule ran tiles {substituted} instead")
    for act in (0, 1):
        assert tally[act].ran > 0, f"tile {tile}: every case was refused"
        tally[act].verdict(f"gpu tile {tile} {name} act={'silu' if act else 'none'}")
    return tally


_TILES = [t for fam in ("v2", "v1", "igemm8", "halo", "halo8", "stream", "tp", "c32", "res", "rw2", "rw3", "rs", "rule") for t in _exact.FAMILIES[fam][0]]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("tile", _TILES)
def test_conv_exact_per_element(dev, tile, dtype):
    """Every family by its tile ids x both 16-bit types x _exact.cases(tile) x {no activation, SiLU}, the shortcut on every other launch.
    No activation: bit-identical to the once-rounded float64 reference.  SiLU: N = 1 ulp, |mean signed error| <= 0.1 ulp per case (tile and type), and separately over its small maps and over its large map.
    MEASURED on the parent commit (MI355X), SiLU, worst ulp | largest |mean signed error| in ulp over the family's tiles (no activation: 0 ulp everywhere, as asserted):
        family                      fp16               bf16
        4-wave v2                   1 | 0.014          0 | 0.031
        register-staged             1 | 0.011          0 | 0.024
        igemm8                      1 | 0.014          0 | 0.031
        halo                        0 | 0.017          0 | 0.032
        halo8                       0 | 0.017          0 | 0.032
        streaming 1x1               1 | 0.012          0 | 0.033
        row-transposed              1 | 0.014          0 | 0.031
        conv3x3_c32                 0 | 0.002          0 | 0.005
        res (132 / 133)             0 | 0.007          0 | 0.020
        rw2 (134)                   0 | 0.021          0 | 0.047
        rw3 (135)                   0 | 0.024          0 | 0.050
        rs (137 / 138)              0 | 0.026          0 | 0.047
        library rule (0)            1 | 0.011          0 | 0.024
    Largest |mean| of a group (small maps / the 17 x 33 map): 0.036 in fp16 (rw3), 0.051 in bf16 (rw3).
    The means are those of a correctly rounding kernel on these operands (the pre-activations are multiples of 1/8: a few hundred distinct values, whose rounding errors
    do not average out completely); a truncating pack measures -0.2 ... -0.5.  Tiles 133 / 134 / 135 / 137 / 138 take SiLU only: their identity-activation launches are
    refused, and the tile the library's rule runs instead (132 or the shape heuristic, recorded from plan.meta and printed) is checked in their place."""
    _run_tile(dev, tile, dtype)


@pytest.mark.parametrize("tile", _exact.F32_TILES + [0])
def test_conv_exact_per_element_fp32(dev, tile):
    """fp32 mode (csrc/conv_f32_pipe.hip, tiles 201-206 and the library's shape rule): exact operands leave nothing to round without an activation -- bit-identical, shortcut
    included; SiLU (expf and a true division, like torch's CPU kernel) within N ulp of fp32 of the float64 reference, with the shortcut on every other launch (SiLU + shortcut
    cancels, so there the distance is in ulps at max(|SiLU|, |sum|) and the bound is N + 1: SiLU's N ulp, then the addition's own rounding against the reference's single one).
    MEASURED on the parent commit (MI355X): without the shortcut worst 1 ulp of fp32, largest |mean signed error| 0.018 ulp -> N = 1; with it worst 1.25 ulp (bound 2)."""
    _run_tile(dev, tile, F32)


@pytest.mark.parametrize("tile", [153, 154])
def test_unknown_row_transposed_ids_are_refused(dev, tile):
    """the 15x range has no variants 13 / 14: refused with YMI_EINVAL, nothing written"""
    from yolort_amd import engine
    got, _ = _launch(dev, engine.Plan(dev, F16), F16, tile, (2, 3, 3, 32, 32, 1, 1), 1, False)
    assert got is None


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("tile", [0, 121, 21, -1])
def test_silu_over_the_whole_domain(dev, tile, dtype):
    """Every finite fp16 value (bf16: every finite value with |v| <= 2^17) as the pre-activation, through ONE identity 1x1 convolution per tile: the library's choice, the
    streaming kernel (lean epilogue, silu_pair), a 4-wave tile and the register-staged kernel (general epilogue).  Rows +-88, +-89, +-104 (exp2 overflows to inf below
    -88.7: rcp(inf) = 0 and the result is -0; it underflows above 88.7), -inf (NaN), the largest pre-activation that rounds to the fp16 maximum and the first that rounds
    to +inf, and the subnormal fp16 results.  torch's fp32 SiLU, then .to(dtype), decides NaN / +-0 / +-inf; finite results within N = 1 ulp of float64 SiLU rounded once.
    MEASURED on an MI355X, worst ulp | mean signed ulp, the four tiles alike: fp16 1 | +0.0004 (127 168 values), bf16 1 | +0.0015 (73 920 values).
    FOUND by this test and fixed with it (csrc/conv_common.hpp, silu<DT> / silu_pair<DT>): for the bf16 pre-activations -87.5, -88 and -88.5 the denominator 1 + exp(-v) lies
    in (2^126, 2^128), its reciprocal is a subnormal fp32 number, v_rcp_f32 flushed it to zero and -0 was stored where SiLU is -8.7e-37 / -5.3e-37 / -3.2e-37 (221 ulp of
    bf16; torch's x / (1 + exp(-x)) keeps them).  The bf16 epilogues now scale numerator and denominator by 1/4; fp16 stores -0 for these either way."""
    from yolort_amd import engine
    x, wt, bias, pre = _exact.silu_domain_problem(dtype)
    npix = x.shape[0]
    plan = engine.Plan(dev, dtype)
    xv = plan.alloc(1, 1, npix, 32)
    xv.as_tensor().copy_(x.view(1, 1, npix, 32).to(dev))
    pc = engine.PackedConv(wt.float().view(64, 32, 1, 1), bias.float(), None, dtype, dev)
    y = plan.conv(xv, pc, 1, 0, tile=tile)
    plan.run()
    torch.cuda.synchronize()
    got = y.as_tensor().cpu().reshape(-1)
    label = f"silu domain tile {tile} (ran {plan.meta[0]['tile']}) {dtype}"
    worst, mean, cnt = _exact.assert_act_domain(got, pre.reshape(-1), "silu", dtype, 1, label)
    print(f"EXACT gpu {label}: worst {worst:.3f} ulp, mean signed {mean:+.4f} ulp over {cnt} values")
    assert abs(mean) <= 0.1
    if dtype == F16:
        assert int(((got.float().abs() > 0) & (got.float().abs() < 2.0 ** -14)).sum()) > 1000   # subnormal results are part of the domain


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("act_name", ["hardswish", "leaky"])
def test_legacy_activations_over_the_whole_domain(dev, act_name, dtype):
    """ymi_act (the launch after an r3.1 convolution) over the same domain, -inf and -0 included: class as torch's fp32 function stores it, finite results within 1 ulp of the
    float64 function rounded once.  MEASURED on the parent commit (MI355X): 0 ulp for both functions and types (bit-identical), |mean signed error| <= 0.0007 ulp."""
    from yolort_amd import _lib
    from yolort_amd._lib import ACT_HARDSWISH, ACT_LEAKY, dtype_code
    lib = _lib.load(require_gpu=True)
    pre = torch.cat([_exact.act_domain(dtype), torch.full((32,), float("-inf"), dtype=dtype)])
    buf = pre.clone().view(-1, 32).to(dev)
    rc = lib.ymi_act(buf.data_ptr(), 32, buf.shape[0], 32, dtype_code(dtype), ACT_HARDSWISH if act_name == "hardswish" else ACT_LEAKY, None, 0, _lib.stream_ptr())
    assert rc == 0, lib.ymi_last_error()
    torch.cuda.synchronize()
    worst, mean, cnt = _exact.assert_act_domain(buf.cpu().reshape(-1), pre.double(), act_name, dtype, 1, f"ymi_act {act_name} {dtype}")
    print(f"EXACT gpu ymi_act {act_name} {str(dtype)[6:]}: worst {worst:.3f} ulp, mean signed {mean:+.4f} ulp over {cnt} values")
    assert abs(mean) <= 0.1
