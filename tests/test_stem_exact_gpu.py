"""Per-element, rounding-level checks of the network's FIRST layer on the GPU (operands, shapes and guard bands: tests/_stem_cases.py; ulp machinery: tests/_exact.py;
the CPU half runs the same forms through the lane simulator, tests/test_hipsim_kernels.py).

The first layer has the most special code of the library -- conv_stem_kernel (tile 41, NHWC4 canvas as 8-channel super-pixels), conv_stem_planar_kernel (persistent,
double-buffered, R/G/B planes gathered from LDS, 32 image pointers per launch), the generic tiles on the 6x3 stride (2,1) pad (2,1) cin-8 im2col form, the fp32 mode's
im2col-table form, Focus.stem_weight(), and stem + body.1 as one launch (csrc/stem_body1_fused.hip, planar and canvas) -- and _exact.WIDTHS has no cin-3 case.  Here
  * without an activation every output equals the float64 reference, rounded ONCE, bit for bit (fp32 output: nothing to round);
  * with SiLU every element is within 1 ulp and the mean signed error within 0.1 ulp, per case and per group of maps (the stem kernels share conv_common.hpp's epilogues);
  * the canvas, every planar image and the output are interior views of larger tensors filled with NaN bit patterns, the output also a channel slice of a wider buffer:
    every guard element and every foreign channel keeps its bits, the output holds no NaN;
  * a form that does not take a shape refuses it with YMI_EINVAL and writes nothing."""
import ctypes as C

import pytest
import torch

import _exact
import _stem_cases as S

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
_NAME = {F16: "fp16", BF16: "bf16", F32: "fp32"}


@pytest.fixture(scope="module")
def dev():
    from yolort_amd import _lib
    _lib.load(require_gpu=True)
    return torch.device("cuda:0")


_PACKED = {}


def _packed(key, make):
    if key not in _PACKED:
        _PACKED[key] = make()
    return _PACKED[key]


def _stem_pc(dev, dtype, wt, bias, key):
    from yolort_amd import engine
    return _packed(("stem", dtype) + key, lambda: engine.PackedConv(wt.float(), bias.float(), None, dtype, dev, stem_superpixel=True))


def _view(g):
    from yolort_amd import engine
    return engine.View(g.t, g.off, g.n, g.h, g.w, g.c, g.cs, g.tail)


def _out_guard(dev, n, ho, wo, cout, dtype, dense=False):
    """the output: an interior view of a NaN-filled tensor and (unless `dense`) channels [16, 16 + cout) of pixels cout_pad8 + 32 wide"""
    if dense:
        return S.Guard(n, ho, wo, cout, dtype, dev).snapshot()
    return S.Guard(n, ho, wo, cout, dtype, dev, c0=16, cs=(cout + 7) // 8 * 8 + 32).snapshot()


def _refused(e, label, *guards):
    assert "(code -1)" in str(e), f"{label}: a refusal carries YMI_EINVAL: {e}"
    torch.cuda.synchronize()
    for g in guards:
        g.assert_untouched(label + " (refused)")


def _canvas_launch(dev, plan, dtype, x, pc, act, tile, out_dtype=None, cv=None):
    """the stem through Plan.conv from the guarded NHWC4 canvas -> ((n, ho, wo, cout) output on the CPU or None when refused, tile recorded in plan.meta)"""
    from yolort_amd._lib import ACT_NONE, ACT_SILU, YmiError
    n, _, h, w = x.shape
    ho, wo = S.stem_hw(h, w)
    cv = S.canvas(x, dtype, dev) if cv is None else cv
    og = _out_guard(dev, n, ho, wo, pc.cout, out_dtype or dtype)
    op = plan.num_ops
    plan.conv(_view(cv), pc, 2, 2, act=ACT_SILU if act else ACT_NONE, out=_view(og), tile=tile)
    ran = plan.meta[op]["tile"]
    label = f"canvas tile {tile} (ran {ran}) {_NAME[dtype]} {(n, h, w)} cout {pc.cout}"
    try:
        plan.run(op, op + 1)
    except YmiError as e:
        _refused(e, label, og, cv)
        return None, ran
    torch.cuda.synchronize()
    og.assert_only_the_view_written(label)
    cv.assert_untouched(label + ": the canvas")       # (its fourth channel is still 0)
    return og.view().cpu(), ran


def _planar_launch(dev, dtype, x, pc, act, out_dtype=None):
    """the stem through Plan.stem_from_planar, a plan whose only op is the stem; the canvas the descriptor names is all NaN: it is not read"""
    from yolort_amd import engine
    from yolort_amd._lib import ACT_NONE, ACT_SILU
    n, _, h, w = x.shape
    ho, wo = S.stem_hw(h, w)
    plan = engine.Plan(dev, dtype)
    cv = S.Guard(n, h, w, 4, dtype, dev).snapshot()
    og = _out_guard(dev, n, ho, wo, pc.cout, out_dtype or dtype)
    imgs, store = S.planar_images(x, dtype, dev)
    before = store.clone()
    plan.conv(_view(cv), pc, 2, 2, act=ACT_SILU if act else ACT_NONE, out=_view(og), tile=41)
    assert plan.stem_from_planar(imgs) == 1
    torch.cuda.synchronize()
    label = f"planar {_NAME[dtype]} {(n, h, w)} cout {pc.cout}"
    og.assert_only_the_view_written(label)
    assert torch.equal(S.bits(store), S.bits(before)), label
    return og.view().cpu()


# ---- 3.1 the canvas form, every tile id -------------------------------------------------------------------------------------------
# ids of test_stem_superpixel (0, 13, 23, 26, 41, -100), then every id of the v2, v1, igemm8 and tp families
_MUST_RUN = {0: S.COUTS, 41: S.COUTS, -100: S.COUTS, 13: [16, 32], 23: [16, 32], 26: [16, 32]}
_TILES = [41, 0, 13, 23, 26, -100] + [t for fam in ("v2", "v1", "igemm8", "tp") for t in _exact.FAMILIES[fam][0]]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("tile", _TILES)
def test_stem_canvas_exact_per_element(dev, tile, dtype):
    """Plan.conv with PackedConv(..., stem_superpixel=True): every shape x cout 16 / 32 / 48 / 64 x every weight set (all 108 taps) x {no activation, SiLU}, and the ODT = F32
    instantiations (out_dtype=torch.float32, no activation: bit-identical with nothing to round) on the first weight set of each cout.
    No activation: bit-identical to the once-rounded float64 reference.  SiLU: N = 1 ulp, |mean signed error| <= 0.1 ulp per case and per group (small / large maps).
    A tile that refuses the form returns YMI_EINVAL and writes nothing; ids 0, 41, -100 (every cout) and 13, 23, 26 (cout <= 32) must run.
    WHICH IDS RAN (MI355X, both types alike): 41, 0, 13, 23, 26, -100, the v2 tiles 12, 21, 24, 27 and the register-staged -1 ... -5 ran every case (tiles 13 / 23 / 26 at
    cout 48 / 64 too); the software-pipelined v2 tiles 61, 64, 66, the 8-wave tiles 111-116 and the row-transposed 141-145, 151, 152, 155 do not take the cin-8 im2col-table form and
    refused every case with YMI_EINVAL, nothing written.
    MEASURED on the commit that added this file (MI355X), the ids that ran all alike (same K order on these operands, same epilogue), worst ulp | |mean signed error|
    | largest |mean| of a group:    no activation  fp16 0 | 0.007 | 0.008   bf16 0 | 0.009 | 0.011   fp32 output 0 | 0 | 0
                                    SiLU           fp16 0 | 0.035 | 0.037   bf16 0 | 0.047 | 0.052"""
    from yolort_amd import engine
    plan = engine.Plan(dev, dtype)
    tally = {0: _exact.Tally(), 1: _exact.Tally(), "f32": _exact.Tally()}
    ran_ids = set()
    for shape in S.SHAPES:
        for cout in S.COUTS:
            for seed in range(S.SETS[cout]):
                x, wt, bias = S.stem_operands(*shape, cout, seed)
                pc = _stem_pc(dev, dtype, wt, bias, (shape, cout, seed))
                cv = S.canvas(x, dtype, dev)
                for mode in (0, 1) + (("f32",) if seed == 0 else ()):
                    act = mode == 1
                    got, ran = _canvas_launch(dev, plan, dtype, x, pc, act, tile, F32 if mode == "f32" else None, cv)
                    if got is None:
                        assert cout not in _MUST_RUN.get(tile, []), f"tile {tile} refused the stem at cout {cout} {shape}"
                        tally[mode].refused += 1
                        continue
                    ran_ids.add(ran)
                    odt = F32 if mode == "f32" else dtype
                    tally[mode].check(got, S.stem_reference64(*shape, cout, seed, act), odt, 1 if act else 0,
                                      f"canvas tile {tile} (ran {ran}) {_NAME[dtype]} {shape} cout {cout} set {seed} mode {mode}", group=S.group_of(shape))
    print(f"STEM canvas tile {tile} {_NAME[dtype]}: ran as {sorted(ran_ids)}")
    for mode in (0, 1, "f32"):
        tally[mode].verdict(f"gpu stem canvas tile {tile} {_NAME[dtype]} mode {mode}")
    if tile in _MUST_RUN:
        assert tally[0].ran > 0 and tally[1].ran > 0


# ---- 3.2 the planar form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("cout", S.COUTS)
def test_stem_planar_exact_per_element(dev, cout, dtype):
    """Plan.stem_from_planar (conv_stem_planar_kernel) on every planar-capable shape, 16-bit and fp32 output: the bounds of the canvas form, and equal to the canvas form
    with tile 41 bit for bit.  The images are carved at 16-byte-aligned offsets out of one NaN-filled tensor; the canvas the descriptor names is all NaN (never read).
    MEASURED (MI355X), SiLU, worst ulp | largest |mean signed error| over the couts | largest |mean| of a group: fp16 0 | 0.040 | 0.043, bf16 0 | 0.051 | 0.054; no activation and
    fp32 output: 0 ulp, as asserted."""
    from yolort_amd import engine
    plan41 = engine.Plan(dev, dtype)
    tally = {0: _exact.Tally(), 1: _exact.Tally(), "f32": _exact.Tally()}
    for shape in [s for s in S.SHAPES if S.planar_ok(s)]:
        for seed in range(S.SETS[cout]):
            x, wt, bias = S.stem_operands(*shape, cout, seed)
            pc = _stem_pc(dev, dtype, wt, bias, (shape, cout, seed))
            for mode in (0, 1, "f32"):
                act, odt = mode == 1, (F32 if mode == "f32" else dtype)
                got = _planar_launch(dev, dtype, x, pc, act, odt)
                label = f"planar {_NAME[dtype]} {shape} cout {cout} set {seed} mode {mode}"
                tally[mode].check(got, S.stem_reference64(*shape, cout, seed, act), odt, 1 if act else 0, label, group=S.group_of(shape))
                twin, _ = _canvas_launch(dev, plan41, dtype, x, pc, act, 41, odt)
                assert torch.equal(S.bits(got), S.bits(twin)), f"{label}: differs from the canvas form (tile 41)"
    for mode in (0, 1, "f32"):
        tally[mode].verdict(f"gpu stem planar {_NAME[dtype]} cout {cout} mode {mode}")


# ---- 3.3 fp32 mode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", _exact.F32_TILES + [0, "v1"])
def test_stem_exact_per_element_fp32(dev, tile, monkeypatch):
    """fp32 mode (Plan(dev, torch.float32): the im2col-table form of csrc/conv_f32_pipe.hip, tiles 201-206 and the library's choice; "v1": the register-staged kernel,
    YOLORT_AMD_F32_V1=1 set before the plan is built): no activation bit-identical, SiLU within N = 1 ulp of fp32, |mean| <= 0.1 (test_conv_exact_per_element_fp32).
    MEASURED (MI355X), the eight forms alike: SiLU worst 1 ulp of fp32, mean signed +0.037 ulp (small maps +0.044, large maps +0.033); no activation 0 ulp."""
    from yolort_amd import engine
    if tile == "v1":
        monkeypatch.setenv("YOLORT_AMD_F32_V1", "1")
    plan = engine.Plan(dev, F32)
    assert plan.use_v1 == (tile == "v1")
    tally = {0: _exact.Tally(), 1: _exact.Tally()}
    for shape in S.SHAPES:
        for cout in S.COUTS:
            for seed in range(S.SETS[cout]):
                x, wt, bias = S.stem_operands(*shape, cout, seed)
                pc = _stem_pc(dev, F32, wt, bias, (shape, cout, seed))
                cv = S.canvas(x, F32, dev)
                for act in (0, 1):
                    got, ran = _canvas_launch(dev, plan, F32, x, pc, act, 0 if tile == "v1" else tile, None, cv)
                    assert got is not None, (tile, shape, cout)
                    tally[act].check(got, S.stem_reference64(*shape, cout, seed, bool(act)), F32, 1 if act else 0,
                                     f"fp32 tile {tile} (ran {ran}) {shape} cout {cout} set {seed} act {act}", group=S.group_of(shape))
    for act in (0, 1):
        tally[act].verdict(f"gpu stem fp32 tile {tile} act {act}")


# ---- 3.4 Focus through the product module -------------------------------------------------------------------------------------------
def _focus_module(version, cout, wt, bias, dev):
    """Focus(3, cout, k=3) whose BatchNorm fold is EXACT: gamma = sqrt(var + eps) computed as PackedConv computes it (scale = gamma / gamma = 1.0), mean 0, beta = bias"""
    from yolort_amd.v5.models.common import Focus
    m = Focus(3, cout, k=3, version=version).eval()
    bn = m.conv.bn
    with torch.no_grad():
        m.conv.conv.weight.copy_(wt.float())
        var = bn.running_var.detach().to(device=dev, dtype=torch.float32)
        bn.weight.copy_(torch.sqrt(var + float(bn.eps)).cpu())
        bn.running_mean.zero_()
        bn.bias.copy_(bias.float())
    return m


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("version", ["r4.0", "r3.1"])
def test_focus_exact_against_the_reference_formulation(dev, version, dtype):
    """Focus(3, 32, k=3) of r4.0 (SiLU in the epilogue) and r3.1 (Hardswish as its own ymi_act launch) emitted into a plan, exact 3x3x12 operands (4 weight sets: all 108
    taps), against F.conv2d(focus_transform(x), W3, b, 1, 1) in float64 -- the reference formulation, not the 6x6 form, so a slot-order error of Focus.stem_weight() fails here.
    Every even-sized shape.  SiLU: 1 ulp, |mean| <= 0.1; Hardswish: 1 ulp of hardswish64 over the ONCE-rounded pre-activation (the bound of
    test_legacy_activations_over_the_whole_domain; the convolution's own output is bit-identical, which the identity-activation launch of the same module asserts).
    MEASURED (MI355X), worst ulp | |mean signed error|: SiLU fp16 0 | 0.035, bf16 0 | 0.046; Hardswish fp16 0 | 0.018, bf16 0 | 0.016; no activation 0 ulp."""
    from yolort_amd import engine
    from yolort_amd._lib import ACT_SILU
    plan = engine.Plan(dev, dtype)
    cout = 32
    tally = {"none": _exact.Tally(), "act": _exact.Tally()}
    hsw64 = _exact.ACT_REFS["hardswish"][0]
    for shape in [s for s in S.SHAPES if s[1] % 2 == 0]:
        n, h, w = shape
        for seed in range(S.SETS[cout]):
            x, wt, bias = S.focus_operands(*shape, cout, seed)
            pre = S.focus_pre64(*shape, cout, seed)
            m = _focus_module(version, cout, wt, bias, dev)
            pc = m.packed(dtype, dev)
            # the fold is exact: the packed weights carry the 6x6 rearrangement's bits (checked against the REFERENCE side: conv over the rearranged image == 6x6 conv)
            w6 = pc.w[:cout, :144].float().cpu().view(cout, 6, 3, 2, 4)
            assert float(w6[..., 3].abs().max()) == 0 and torch.equal(pc.bias[:cout].cpu().double(), bias)
            w6 = w6[..., :3].reshape(cout, 6, 6, 3).permute(0, 3, 1, 2).double()
            assert torch.equal(torch.nn.functional.conv2d(x, w6, bias, 2, 2), pre), "the packed weights do not carry the intended bits"
            cv = S.canvas(x, dtype, dev)
            for which in ("none", "act"):
                og = _out_guard(dev, n, h // 2, w // 2, cout, dtype)
                op = plan.num_ops
                if which == "none":
                    act_saved, m.conv.act = m.conv.act, torch.nn.Identity()
                m.emit(plan, _view(cv), out=_view(og))
                if which == "none":
                    m.conv.act = act_saved
                plan.run(op, plan.num_ops)
                torch.cuda.synchronize()
                label = f"focus {version} {_NAME[dtype]} {shape} set {seed} {which}"
                assert plan.num_ops - op == (2 if (which == "act" and version == "r3.1") else 1), label
                og.assert_only_the_view_written(label)
                cv.assert_untouched(label)
                p = pre.permute(0, 2, 3, 1).contiguous()
                if which == "none":
                    ref, ulp = p, 0
                elif version == "r4.0":
                    assert plan.conv_descs[op].act == ACT_SILU
                    assert not bool(((p < -80) & (p > -300)).any())
                    ref, ulp = _exact.silu64(p), 1
                else:
                    ref, ulp = hsw64(_exact.round_once(p, dtype).double()), 1
                tally[which].check(og.view().cpu(), ref, dtype, ulp, label, group=S.group_of(shape))
    for which in tally:
        tally[which].verdict(f"gpu focus {version} {_NAME[dtype]} {which}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _two_op_plan(dev, dtype, x, w0, b0, w1, b1, tile0=41, stem_cout=32, res=False):
    """plan of stem (SiLU) + Conv(32, 64, 3, 2, 1) (tile 131) over guarded buffers -> (plan, canvas, stem output, body.1 output)"""
    from yolort_amd import engine
    n, _, h, w = x.shape
    hs, ws = S.stem_hw(h, w)
    ho, wo = S.body1_hw(hs, ws)
    plan = engine.Plan(dev, dtype)
    cv = S.canvas(x, dtype, dev)
    pc0 = engine.PackedConv(w0.float(), b0.float(), None, dtype, dev, stem_superpixel=True)
    pc1 = engine.PackedConv(w1.float(), b1.float(), None, dtype, dev)
    sg = _out_guard(dev, n, hs, ws, stem_cout, dtype, dense=True)
    og = _out_guard(dev, n, ho, wo, 64, dtype)
    plan.conv(_view(cv), pc0, 2, 2, out=_view(sg), tile=tile0)
    rv = None
    if res:
        rv = plan.alloc(n, ho, wo, 64, zero=True)
    if stem_cout == 32:
        plan.conv(_view(sg), pc1, 2, 1, out=_view(og), res=rv, tile=131)
    return plan, cv, sg, og


def _ptrs(imgs):
    return (C.c_void_p * len(imgs))(*[im.data_ptr() for im in imgs])


def test_stem_entry_points_refuse_what_they_cannot_take(dev):
    """YMI_EINVAL with nothing written: planar and planar-fused with W % 8 != 0; an image pointer offset by 2 bytes; ymi_stem_body1 / ymi_stem_body1_planar called directly
    with a stem of cout 64; the same entry points with a body.1 that has a shortcut"""
    from yolort_amd import _lib
    from yolort_amd._lib import YmiError
    lib = _lib.load(require_gpu=True)
    dtype = F16

    def refused(rc_or_call, label, *guards):
        if callable(rc_or_call):
            with pytest.raises(YmiError) as e:
                rc_or_call()
            _refused(e.value, label, *guards)
        else:
            assert rc_or_call == -1, f"{label}: expected YMI_EINVAL, got {rc_or_call}: {lib.ymi_last_error().decode()}"
            torch.cuda.synchronize()
            for g in guards:
                g.assert_untouched(label)

    # W % 8 != 0: the stem alone, and stem + body.1
    shape = (2, 7, 10)
    x, wt, bias = S.stem_operands(*shape, 32, 0)
    w1, b1 = S.body1_weights()
    imgs, _ = S.planar_images(x, dtype, dev)
    assert all(im.data_ptr() % 16 == 0 for im in imgs[:1])
    plan, cv, sg, og = _two_op_plan(dev, dtype, x, wt, bias, w1, b1)
    assert plan.stem_body1_fusable()
    refused(lambda: plan.stem_from_planar(imgs), "planar-fused, W % 8 != 0", sg, og)
    refused(lib.ymi_conv_stem_planar(C.byref(plan.conv_descs[0]), _ptrs(imgs), len(imgs), _lib.stream_ptr()), "planar, W % 8 != 0", sg, og)
    # an image pointer offset by 2 bytes
    shape = (2, 7, 16)
    x, wt, bias = S.stem_operands(*shape, 32, 0)
    good, _ = S.planar_images(x, dtype, dev)
    odd, _ = S.planar_images(x, dtype, dev, shift=1)
    assert odd[1].data_ptr() % 16 == 2
    plan, cv, sg, og = _two_op_plan(dev, dtype, x, wt, bias, w1, b1)
    refused(lambda: plan.stem_from_planar([good[0], odd[1]]), "planar-fused, image 1 offset by 2 bytes", sg, og)
    refused(lib.ymi_conv_stem_planar(C.byref(plan.conv_descs[0]), _ptrs([good[0], odd[1]]), 2, _lib.stream_ptr()), "planar, image 1 offset by 2 bytes", sg, og)
    # body.1 with a shortcut
    plan, cv, sg, og = _two_op_plan(dev, dtype, x, wt, bias, w1, b1, res=True)
    assert plan.conv_descs[1].res and not plan.stem_body1_fusable()
    refused(lib.ymi_stem_body1(C.byref(plan.conv_descs[0]), C.byref(plan.conv_descs[1]), _lib.stream_ptr()), "ymi_stem_body1, body.1 with a shortcut", sg, og)
    refused(lib.ymi_stem_body1_planar(C.byref(plan.conv_descs[0]), C.byref(plan.conv_descs[1]), _ptrs(good), 2, _lib.stream_ptr()), "ymi_stem_body1_planar, body.1 with a shortcut", sg, og)
    # a stem of cout 64 (body.1's descriptor is taken from a valid pair: the stem's is what is wrong)
    d1 = _two_op_plan(dev, dtype, x, wt, bias, w1, b1)
    x64, wt64, bias64 = S.stem_operands(*shape, 64, 0)
    plan64, cv64, sg64, _ = _two_op_plan(dev, dtype, x64, wt64, bias64, w1, b1, stem_cout=64)
    body1 = d1[0].conv_descs[1]
    refused(lib.ymi_stem_body1(C.byref(plan64.conv_descs[0]), C.byref(body1), _lib.stream_ptr()), "ymi_stem_body1, stem of cout 64", sg64, d1[3])
    refused(lib.ymi_stem_body1_planar(C.byref(plan64.conv_descs[0]), C.byref(body1), _ptrs(good), 2, _lib.stream_ptr()), "ymi_stem_body1_planar, stem of cout 64", sg64, d1[3])


# ---- 4. stem + body.1 as one launch -------------------------------------------------------------------------------------------------
def _fused_and_separate(dev, dtype, x, w0, b0, w1, b1, form, monkeypatch, label):
    """body.1's output from the ONE launch (`form`: "planar" -- stem_from_planar returning 2 -- or "canvas" -- set_fuse_stem(True), run(0, 2)) and from the two launches
    (the form's stem kernel, then tile 131): asserts the guard bands and that the fused launch leaves the stem's output buffer untouched -> (fused, separate) on the CPU"""
    outs = {}
    for fused in (False, True):
        plan, cv, sg, og = _two_op_plan(dev, dtype, x, w0, b0, w1, b1)
        if form == "planar":
            imgs, store = S.planar_images(x, dtype, dev)
            cv.view().copy_(torch.full_like(cv.view(), float("nan")))     # not read on the planar paths
            monkeypatch.setenv("YOLORT_AMD_FUSE_STEM", "1" if fused else "0")
            covered = plan.stem_from_planar(imgs)
            assert covered == (2 if fused else 1), label
            plan.run(covered, 2)
        else:
            assert plan.set_fuse_stem(fused) == fused, label
            plan.run(0, 2)
        torch.cuda.synchronize()
        og.assert_only_the_view_written(f"{label} fused={fused}")
        if fused:
            sg.assert_untouched(f"{label}: the stem's output buffer")
        else:
            sg.assert_only_the_view_written(f"{label}: the stem's output")
        outs[fused] = og.view().cpu()
    monkeypatch.delenv("YOLORT_AMD_FUSE_STEM", raising=False)
    return outs[True], outs[False]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("form", ["planar", "canvas"])
def test_fused_stem_body1_exact(dev, form, dtype, monkeypatch):
    """csrc/stem_body1_fused.hip, both input forms, every shape the form takes (canvas: all; planar: W % 8 == 0):
      * BIT IDENTITY with the two launches on the exact stem operands (cout 32, all 4 weight sets, SiLU) followed by an exact Conv(32, 64, 3, 2, 1); the stem's output buffer
        stays untouched, the guard bands hold;
      * an INDEPENDENT two-layer reference on the problem whose intermediate is exact (_stem_cases.two_layer_operands: stem pre-activations are integers in [19, 61] that SiLU
        and the rounding leave alone; body.1 pads with 0, not 40): within N = 1 ulp of float64 SiLU rounded once, |mean signed error| <= 0.1 ulp, for the one launch AND for
        the two launches.
    MEASURED (MI355X), the one launch and the two launches alike, planar and canvas alike to the digit shown: worst 0 ulp, mean signed +0.003 ulp (fp16), +0.007 ulp (bf16)."""
    w1, b1 = S.body1_weights()
    tally = {"fused": _exact.Tally(), "two launches": _exact.Tally()}
    for shape in [s for s in S.SHAPES if form == "canvas" or S.planar_ok(s)]:
        for seed in range(S.SETS[32]):
            x, wt, bias = S.stem_operands(*shape, 32, seed)
            label = f"fused {form} {_NAME[dtype]} {shape} set {seed}"
            one, two = _fused_and_separate(dev, dtype, x, wt, bias, w1, b1, form, monkeypatch, label)
            assert torch.equal(S.bits(one), S.bits(two)), f"{label}: differs from the two launches"
        x, w0, b0, w1x, b1x = S.two_layer_operands(*shape)
        label = f"two-layer {form} {_NAME[dtype]} {shape}"
        one, two = _fused_and_separate(dev, dtype, x, w0, b0, w1x, b1x, form, monkeypatch, label)
        ref = S.two_layer_reference64(*shape)
        tally["fused"].check(one, ref, dtype, 1, label + " fused", group=S.group_of(shape))
        tally["two launches"].check(two, ref, dtype, 1, label + " two launches", group=S.group_of(shape))
    for k in tally:
        tally[k].verdict(f"gpu fused stem + body.1 {form} {_NAME[dtype]} {k}")


# ---- 5. the persistent walk and the 32-image groups -----------------------------------------------------------------------------------
_BIG = (33, 128, 512)


@pytest.fixture(scope="module")
def big_refs():
    """float references of the 33-image case, computed once: by the bound of _stem_cases the fp32 F.conv2d is itself exact -- asserted equal to float64 on image 0"""
    import torch.nn.functional as F
    x, wt, bias = S.stem_operands(*_BIG, 32, 0)
    ref32 = F.conv2d(x.float(), wt.float(), bias.float(), 2, 2)
    assert torch.equal(ref32[0].double(), F.conv2d(x[:1], wt, bias, 2, 2)[0])
    x2, w0, b0, w1, b1 = S.two_layer_operands(*_BIG)
    v = F.conv2d(x2[[0, 31, 32]], w0, b0, 2, 2)
    assert torch.equal(v, v.round()) and float(v.min()) >= 19 and float(v.max()) <= 61
    return ref32.permute(0, 2, 3, 1).contiguous(), S.body1_reference64(v, w1, b1)


@pytest.mark.parametrize("form", ["planar", "canvas"])
def test_stem_33_images_walk_the_tiles_and_the_second_group(dev, form, big_refs, monkeypatch):
    """n = 33 images of 128 x 512, cout 32, fp16.  Each launch group of 32 images has 32 * 8 * 8 = 2048 stem tiles against at most 3 * 256 resident blocks of the planar
    kernel (most blocks walk three tiles, both LDS buffers are reused) and 32 * 4 * 8 = 1024 fused tiles against 256 blocks (four tiles each); image 33 goes through the
    second group (PL_MAX / SB_MAX_IMGS), the canvas-fused form takes all 33 in one launch.  The occupancy itself cannot be observed here: only the tile counts are asserted.
    Stem without activation: bit-identical on all 33 images.  Fused: bit-identical to the two launches, and within 1 ulp of the independent reference on images 0, 31, 32.
    MEASURED (MI355X), planar and canvas alike: stem 0 ulp on all 33 images (as asserted); fused worst 0 ulp, mean signed +0.006 ulp over 786 432 elements."""
    from yolort_amd import engine
    n, h, w = _BIG
    hs, ws = S.stem_hw(h, w)
    ho, wo = S.body1_hw(hs, ws)
    assert 32 * ((hs + 7) // 8) * ((ws + 31) // 32) == 2048 and 2048 > 2 * 768 and 32 * ((ho + 7) // 8) * ((wo + 15) // 16) == 1024 == 4 * 256 and n == 32 + 1
    ref32, ref2 = big_refs
    x, wt, bias = S.stem_operands(*_BIG, 32, 0)
    pc = engine.PackedConv(wt.float(), bias.float(), None, F16, dev, stem_superpixel=True)
    if form == "planar":
        got = _planar_launch(dev, F16, x, pc, False)
    else:
        got, ran = _canvas_launch(dev, engine.Plan(dev, F16), F16, x, pc, False, 41)
        assert ran == 41
    want = ref32.to(F16)
    assert torch.equal(S.bits(got), S.bits(want)), f"stem {form}: images {sorted(set((S.bits(got) != S.bits(want)).nonzero()[:, 0].tolist()))} differ from the reference"
    x2, w0, b0, w1, b1 = S.two_layer_operands(*_BIG)
    one, two = _fused_and_separate(dev, F16, x2, w0, b0, w1, b1, form, monkeypatch, f"33 images {form}")
    assert torch.equal(S.bits(one), S.bits(two)), f"fused {form}: images {sorted(set((S.bits(one) != S.bits(two)).nonzero()[:, 0].tolist()))} differ from the two launches"
    worst, mean, cnt = _exact.assert_elementwise(one[[0, 31, 32]], ref2, F16, 1, f"33 images fused {form}")
    print(f"EXACT gpu 33 images fused {form}: worst {worst:.3f} ulp, mean signed {mean:+.4f} ulp over {cnt} elements")
    assert abs(mean) <= 0.1
