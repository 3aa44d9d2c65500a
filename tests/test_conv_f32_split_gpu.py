"""fp32 mode on the 16-bit matrix pipe (csrc/conv_f32_split.hip, tiles 211-216: 6 bf16 products per k, 221-226: 8) against float64, per element, under the error
contract of include/yolort_amd.h ("fp32 mode on the 16-bit matrix pipe"): with S = sum |x||w| over an output's products
    |pre-activation - exact| <= D_NP * S + A_NP * (S + |bias|),  D_6 = 2^-23 + 2^-32, D_8 = 2^-32,  A_NP = 6 sqrt(64 NP + ceil(k_pad / 64) + 1) 2^-24 * 1.016
SiLU (|SiLU'| <= 1.1) within 2 ulp of its own value, the shortcut one more rounding.  The constants are the header's, not fitted to what the kernel gives."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import _exact

pytestmark = pytest.mark.gpu
TILES = [211, 212, 213, 214, 215, 216, 221, 222, 223, 224, 225, 226]
D = {6: 2.0 ** -23 + 2.0 ** -32, 8: 2.0 ** -32}


def _np_of(tile):
    return 6 if tile < 220 else 8


def _bound(tile, k_pad, x, wt, bias, s, p, act, res):
    """(float64 reference, per-element bound), both NHWC"""
    a = 6 * math.sqrt(64 * _np_of(tile) + math.ceil(k_pad / 64) + 1) * 2.0 ** -24 * 1.016
    S = F.conv2d(x.double().abs(), wt.double().abs(), None, s, p)
    ref = F.conv2d(x.double(), wt.double(), bias.double(), s, p)
    e = D[_np_of(tile)] * S + a * (S + bias.double().abs().view(1, -1, 1, 1))
    if act:
        ref = _exact.silu64(ref)
        e = 1.1 * e + 2.0 ** -22 * ref.abs()
    if res is not None:
        ref = ref + res.double()
        e = e + 2.0 ** -24 * ref.abs()
    return ref.permute(0, 2, 3, 1), e.permute(0, 2, 3, 1)


@pytest.fixture(scope="module")
def dev():
    from yolort_amd import _lib
    _lib.load(require_gpu=True)
    return torch.device("cuda:0")


def _launch(dev, tile, x, wt, bias, s, p, act, res=None, split=0, up2=False, dtype=torch.float32, want_tile=None):
    """one Plan.conv launch on NaN-poisoned outputs -> (y, y2 or None) on the CPU, k_pad; `want_tile`: what the plan must record for tile 0 (None: the 20x rule)"""
    from yolort_amd import engine
    plan = engine.Plan(dev, dtype)
    n, cin, h, w = x.shape
    cout = wt.shape[0]
    xv = plan.alloc(n, h, w, cin)
    xv.as_tensor().copy_(x.permute(0, 2, 3, 1).to(dev, dtype))
    pc = engine.PackedConv(wt, bias, None, dtype, dev)
    ho, wo = engine.conv_out_hw(h, w, wt.shape[2:], (s, s), (p, p))
    y = plan.alloc(n, ho, wo, split or cout)
    y2 = plan.alloc(n, 2 * ho, 2 * wo, cout) if up2 else (plan.alloc(n, ho, wo, cout - split) if split else None)
    rv = None
    if res is not None:
        rv = plan.alloc(n, ho, wo, cout)
        rv.as_tensor().copy_(res.permute(0, 2, 3, 1).to(dev, dtype))
    for v in (y, y2):
        if v is not None:
            v.as_tensor().fill_(float("nan"))
    plan.conv(xv, pc, s, p, act=act, out=y, res=rv, tile=tile, out2=None if up2 else y2, split=split, up2_out=y2 if up2 else None)
    assert plan.meta[0]["tile"] == (tile or want_tile or plan.lib.ymi_conv_f32_pick_tile(n * ho * wo, pc.cout_pad))
    plan.run()
    torch.cuda.synchronize()
    return y.as_tensor().cpu(), None if y2 is None else y2.as_tensor().cpu(), pc.k_pad


def _operands(n, cin, cout, h, w, k, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, cin, h, w, generator=g), torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k), torch.randn(cout, generator=g) * 0.1)


def _assert_within(got, ref, e, label):
    d = (got.double() - ref).abs()
    print(f"{label}: worst error / bound {float((d / e).max()):.4f}")
    assert bool(torch.isfinite(got).all()) and bool((d <= e).all()), f"{label}: error / bound {float((d / e).max()):.3f} at {int((d / e).argmax())}"


# 2 x 9 x 11 = 198 pixels: no multiple of any block's M; cin 16 / 48: K of one step (k1) and no multiple of the 4-step fold; cout 8 / 72: ragged N; cin 8: the im2col-table form
@pytest.mark.parametrize("k,s,widths", [(1, 1, [(16, 72), (48, 8)]), (3, 1, [(16, 72), (48, 8)]), (3, 2, [(16, 8), (48, 72)]), (3, 1, [(8, 72)])], ids=["k1s1", "k3s1", "k3s2", "table"])
@pytest.mark.parametrize("tile", TILES)
def test_split_tiles_meet_the_contract_per_element(dev, tile, k, s, widths):
    for i, (cin, cout) in enumerate(widths):
        x, wt, bias = _operands(2, cin, cout, 9, 11, k, seed=tile + cin + k + s)
        y, _, k_pad = _launch(dev, tile, x, wt, bias, s, k // 2, act=i % 2)
        _assert_within(y, *_bound(tile, k_pad, x, wt, bias, s, k // 2, i % 2, None), f"tile {tile} k{k} s{s} {cin}->{cout}")


@pytest.mark.parametrize("form", ["shortcut", "split", "up2"])
@pytest.mark.parametrize("tile", [212, 221])
def test_split_tiles_epilogue_forms(dev, tile, form):
    """shortcut after SiLU; cv1 + cv2 in one launch (channels 40 ... to a second view); the x2-upsampled second output"""
    cout = 64 if form == "up2" else 72
    x, wt, bias = _operands(2, 48, cout, 9, 11, 3, seed=tile)
    res = torch.randn(2, cout, 9, 11, generator=torch.Generator().manual_seed(5)) if form == "shortcut" else None
    y, y2, k_pad = _launch(dev, tile, x, wt, bias, 1, 1, 1, res=res, split=40 if form == "split" else 0, up2=form == "up2")
    ref, e = _bound(tile, k_pad, x, wt, bias, 1, 1, 1, res)
    if form == "split":
        _assert_within(y2, ref[..., 40:], e[..., 40:], f"tile {tile} second view")
        ref, e = ref[..., :40], e[..., :40]
    _assert_within(y, ref, e, f"tile {tile} {form}")
    if form == "up2":
        assert torch.equal(y2, y.repeat_interleave(2, 1).repeat_interleave(2, 2))


def _coherent(shape, seed, e0):
    """positive values 2^e (1 + j / 128 + 2^-8 - 63 * 2^-23), j < 16: 24 significant bits; hi = 2^e (1 + j / 128), mid = 2^(e - 8) (rounded UP from just below),
    lo = -63 * 2^(e - 23), next to the largest |lo| / |v| there is (2^-17) -- and every `lo` has the same sign, so what a split without it loses adds up instead of
    averaging out"""
    g = torch.Generator().manual_seed(seed)
    e, j = torch.randint(e0 - 2, e0 + 1, shape, generator=g).double(), torch.randint(0, 16, shape, generator=g).double()
    v = 2.0 ** e * (1 + j / 128 + 2.0 ** -8 - 63 * 2.0 ** -23)
    assert torch.equal(v.float().double(), v)
    return v.float()


def test_the_np6_bound_rejects_a_two_term_split(dev):
    """the contract is not one a cheaper kernel passes as well: hi + mid alone (float64 on the host) violates the NP = 6 bound on this input, tile 211 meets it"""
    x, wt, bias = _coherent((2, 16, 9, 11), 1, 0), _coherent((72, 16, 3, 3), 2, -3), torch.zeros(72)
    y, _, k_pad = _launch(dev, 211, x, wt, bias, 1, 1, 0)
    ref, e = _bound(211, k_pad, x, wt, bias, 1, 1, 0, None)

    def two(v):
        hi = v.bfloat16().float()
        return (hi + (v - hi).bfloat16().float()).double()
    cheap = F.conv2d(two(x), two(wt), None, 1, 1).permute(0, 2, 3, 1)
    assert float(((cheap - ref).abs() / e).max()) > 1.5
    _assert_within(y, ref, e, "tile 211, coherent lo terms")


@pytest.mark.parametrize("case", [(3, 5, 4, 64, 40, 3, 1), (1, 17, 33, 48, 96, 3, 2), (2, 3, 3, 32, 32, 1, 1)])
def test_bf16_representable_operands_equal_the_fp32_tiles_bit_for_bit(dev, case):
    """small integers (tests/_exact.py): mid = lo = 0 and every sum is exact -- tiles 211 / 221 and the library's fp32 choice store the same bits"""
    x, wt, bias, _ = _exact.exact_operands(*case)
    k, s = case[5:]
    outs = {t: _launch(dev, t, x.float(), wt.float(), bias.float(), s, k // 2, 0)[0] for t in (0, 211, 221)}
    assert float(outs[0].abs().max()) > 0
    assert torch.equal(outs[211], outs[0]) and torch.equal(outs[221], outs[0])


@pytest.mark.parametrize("what", ["fp16 plan", "id 217", "misaligned zero page"])
def test_refusals_are_einval_and_write_nothing(dev, what):
    from yolort_amd import _lib, engine
    dtype = torch.float16 if what == "fp16 plan" else torch.float32
    plan = engine.Plan(dev, dtype)
    xv = plan.alloc(1, 4, 4, 16)
    pc = engine.PackedConv(torch.ones(32, 16, 1, 1), torch.zeros(32), None, dtype, dev)
    y = plan.alloc(1, 4, 4, 32, zero=True)
    for tile in ((217,) if what == "id 217" else (211, 226) if what == "fp16 plan" else (201, 211)):   # the last: refused by tile 201, hence by 211
        d = plan.conv_desc(xv, pc, (1, 1), (0, 0), 1, y, None, tile)
        if what == "misaligned zero page":
            d.zeros += 4
        rc = plan.lib.ymi_conv2d(C.byref(d), None)
        with pytest.raises(_lib.YmiError, match=r"code -1\): ymi_conv2d"):
            _lib.check(rc, "ymi_conv2d")
    torch.cuda.synchronize()
    assert float(y.as_tensor().float().abs().max()) == 0


@pytest.mark.parametrize("env", [{"YOLORT_AMD_F32_SPLIT": "7"}, {"YOLORT_AMD_F32_SPLIT": "6", "YOLORT_AMD_F32_V1": "1"}])
def test_the_switch_refuses_other_values_and_the_register_staged_kernel(dev, env, monkeypatch):
    from yolort_amd import _lib, engine
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(_lib.YmiError, match="YOLORT_AMD_F32_SPLIT"):
        engine.Plan(dev, torch.float32)


@pytest.mark.parametrize("np_,tile", [("6", 212), ("8", 222)])
def test_the_switch_moves_the_shape_rule_to_its_split_tile(dev, np_, tile, monkeypatch):
    monkeypatch.setenv("YOLORT_AMD_F32_SPLIT", np_)
    x, wt, bias = _operands(2, 48, 72, 9, 11, 3, seed=3)
    y, _, k_pad = _launch(dev, 0, x, wt, bias, 1, 1, 1, want_tile=tile)   # 198 pixels x 72 channels: the rule picks 202
    _assert_within(y, *_bound(tile, k_pad, x, wt, bias, 1, 1, 1, None), f"switch {np_}")


@pytest.mark.parametrize("tag", ["n", "s"])
@pytest.mark.parametrize("np_", ["6", "8"])
def test_conditioned_goldens_with_the_switch(dev, tag, np_, monkeypatch):
    """yolov5n / yolov5s in fp32 mode with YOLORT_AMD_F32_SPLIT set, under the fp32-mode assertions of tests/test_golden_gpu.py (IoU >= 1 - 1e-3, equal labels, its score
    tolerance: _assert_fp32 there holds the constants)"""
    import test_golden_gpu as tg
    from workloads.synth import cond_images
    monkeypatch.setenv("YOLORT_AMD_F32_SPLIT", np_)
    meta, ref, _ = tg._golden("cond", tag)
    m = tg._model(meta, dev, torch.float32, "cond")
    got = [tg._np(d) for d in m.predict([im.to(dev) for im in cond_images(meta["arch"], meta["seed"])])]
    tg._assert_fp32(ref, got, meta["thr"], f"cond_{tag} split {np_}")
