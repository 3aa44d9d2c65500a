"""The letterbox, SPP, upsample, view-copy and layout kernels of csrc/preproc_pool.hip without a GPU: the cases of tests/_pre_cases.py on the CPU simulator
(tests/hipsim: preproc_pool.hip is a simulator unit, its entry points take host pointers), the checks that the cases reach what they claim to reach (computed from the
model and the geometry alone), and the letterbox model held to the oracle.  tests/test_pre_exact_gpu.py runs the same cases on the real kernels."""
import numpy as np
import pytest
import torch

import _pre_cases as P
from test_hipsim_kernels import sim  # noqa: F401  (the module-scoped fixture that builds the simulator library)

LB_NAMES = [c.name for c in P.LB_CASES]


@pytest.fixture(scope="module")
def lib(sim):  # noqa: F811
    return P.proto(sim)


# ---- 1. letterbox: the model against the oracle -------------------------------------------------------------------------------------------------------------------------
def test_uint8_widening_covers_all_256_values():
    """float32(v) / float32(255) in NumPy = torch's `u.float() / 255.0` (what the reference's read_image(...) / 255.0 gives), for every value"""
    v = torch.arange(256, dtype=torch.uint8)
    assert np.array_equal(P.lb_widen(v.view(1, 1, 256).expand(3, 1, 256), "u8")[0, 0], (v.float() / 255.0).numpy())
    u8_copies = [c for c in P.LB_CASES if c.name.startswith("copy") and c.in_dt in ("u8", "u8hwc")]
    assert len(u8_copies) == 4
    for c in u8_copies:
        assert len(torch.unique(P.lb_images(c)[0])) == 256, "the first image of a uint8 identity case holds all 256 values"


ORACLE_SETS = ((96, [(135, 101), (60, 80), (90, 160), (47, 63), (100, 37), (81, 60)]), (64, [(23, 97), (40, 201), (5, 7), (64, 64), (64, 48)]), (160, [(31, 17), (160, 3)]))


@pytest.mark.parametrize("size,shapes", ORACLE_SETS, ids=[str(s) for s, _ in ORACLE_SETS])
@pytest.mark.parametrize("in_dt", ["f32", "f16", "bf16", "u8"])
def test_model_is_held_to_the_oracle_letterbox(size, shapes, in_dt):
    """the model (fp32, before narrowing) against O.letterbox on the oracle's own geometry, within lb_oracle_bound; the measured maximum is printed next to the bound"""
    from oracle import yolov5_oracle as O
    imgs = [P.lb_image(in_dt, h, w, seed=h + w) for h, w in shapes]
    wide = [P.lb_widen(im, in_dt) for im in imgs]
    ref, sizes = O.letterbox([torch.from_numpy(x) for x in wide], size, size, 32)
    hb, wb = ref.shape[2:]
    worst = 0.0
    for i, ((h, w), x) in enumerate(zip(shapes, wide)):
        hr, wr = O.resized_hw(h, w, float(size), float(size))
        assert (hr, wr) == tuple(sizes[i])
        pt, pl = O.pad_offsets(hb, hr), O.pad_offsets(wb, wr)
        canvas = np.full((3, hb, wb), np.float32(P.FILL), np.float32)
        canvas[:, pt: pt + hr, pl: pl + wr] = P.lb_resize(x, hr, wr)
        err = float(np.abs(canvas.astype(np.float64) - ref[i].numpy().astype(np.float64)).max())
        print(f"letterbox model vs oracle, {in_dt} {h}x{w} -> {hr}x{wr} on {hb}x{wb}: max |err| {err:.3e} (bound {P.lb_oracle_bound():.3e})")
        worst = max(worst, err)
    assert worst <= P.lb_oracle_bound(), worst


@pytest.mark.parametrize("name", [n for n in LB_NAMES if not n.startswith(("n66", "copy", "empty"))])
def test_model_is_held_to_the_oracle_resize_on_the_case_geometry(name):
    """the same bound on the explicit geometries of the case table (up-scale 8x, down-scale 6x, one-pixel sides), against the oracle's resize"""
    from oracle import yolov5_oracle as O
    case = P.LB_BY_NAME[name]
    for (hin, win, hr, wr, _, _), im in zip(case.geoms, P.lb_images(case)):
        x = P.lb_widen(im, case.in_dt)
        err = float(np.abs(P.lb_resize(x, hr, wr).astype(np.float64) - O.resize_bilinear(torch.from_numpy(x), hr, wr).numpy().astype(np.float64)).max())
        print(f"letterbox model vs oracle resize, {name} {hin}x{win} -> {hr}x{wr}: max |err| {err:.3e} (bound {P.lb_oracle_bound():.3e})")
        assert err <= P.lb_oracle_bound(), err


# ---- 1. letterbox: the cases reach what they claim --------------------------------------------------------------------------------------------------------------------
def _tiled(case):
    return [d for d in P.lb_dispatch(case) if d[0] == "tile"]


def test_case_table_covers_what_the_issue_lists():
    pairs = {(c.in_dt, c.out_dt) for c in P.LB_CASES if c.name.startswith("io-")}
    assert pairs == {(i, o) for i in P.IN_DTS for o in P.OUT_DTS}
    assert {c.c_out for c in P.LB_CASES} == {4, 5, 8}
    for case in P.LB_CASES:
        for hin, win, hr, wr, pt, pl in case.geoms:
            assert min(hin, win, hr, wr) >= 1 and pt >= 0 and pl >= 0 and pt + hr <= case.hb and pl + wr <= case.wb, case.name
        assert 32 <= case.hb <= 64 and (case.wb == 32 or 160 <= case.wb <= 288), case.name
    up = P.LB_BY_NAME["up-u8"].geoms[0]
    assert up[2] / up[0] >= 4 and up[3] / up[1] >= 4
    assert P.LB_BY_NAME["w161-identity"].wb % 2 == 1 and P.LB_BY_NAME["w162-identity"].wb % 4 == 2
    for name in ("one-win", "one-hin", "one-hr", "one-wr"):
        g = P.LB_BY_NAME[name].geoms[0]
        assert g[{"one-hin": 0, "one-win": 1, "one-hr": 2, "one-wr": 3}[name]] == 1 and sorted(g[:4])[1] > 1
    g = P.LB_BY_NAME["edge-first-col"].geoms[0]
    assert (g[5] + g[3] - 1) % P.LB_TW == 0
    g = P.LB_BY_NAME["edge-last-col"].geoms[0]
    assert (g[5] + g[3] - 1) % P.LB_TW == P.LB_TW - 1
    assert any(g[4] % 2 and g[5] % 2 for c in P.LB_CASES for g in c.geoms)


def test_identity_cases_take_the_copy_kernel_on_both_of_its_paths():
    for wb, px in ((160, 8), (164, 4)):
        cases = [c for c in P.LB_CASES if c.name.startswith(f"copy{wb}-")]
        assert {c.in_dt for c in cases} == {"f16", "bf16", "f32", "u8", "u8hwc"}
        for c in cases:
            assert P.lb_dispatch(c) == [("copy", px)]
            vec = [g for g in c.geoms if g[1] % px == 0 and g[5] % px == 0]
            assert vec and len(vec) < len(c.geoms), "vector groups and scalar groups"
            assert any(g[1] % 8 == 0 and g[5] % 8 == 0 for g in c.geoms) and any(g[1] % 4 == 0 and g[5] % 4 == 0 and (g[1] % 8 or g[5] % 8) for g in c.geoms)
            assert any(g[1] % 4 and g[5] % 4 for g in c.geoms)
    for name in ("w161-identity", "w162-identity"):   # identity sizes the copy kernel refuses: the resampling kernels at scale 1
        c = P.LB_BY_NAME[name]
        assert all(g[:2] == g[2:4] for g in c.geoms) and P.lb_dispatch(c)[0][0] == "tile"


def test_tiled_cases_have_tiles_that_straddle_the_edge_of_the_resized_region():
    seen = set()
    for case in P.LB_CASES:
        for _, knob, cg in P.LB_VARIANTS:
            for d in P.lb_dispatch(case, knob, cg):
                seen.add(d)
                if d[0] == "tile":
                    assert any(t["straddle"] for t in P.lb_tiles(case, d[1], d[2])), (case.name, d)
    # every template variant of the tiled kernel, both copy widths and the per-pixel kernel are reached
    assert {("tile", r, g) for r in (1, 2, 4) for g in (1, 2)} | {("copy", 8), ("copy", 4), ("pixel",)} <= seen


def test_misaligned_cases_have_a_non_zero_base_alignment():
    mis = [c for c in P.LB_CASES if c.name.startswith("mis-")]
    assert sorted(m for c in mis if c.in_dt == "u8" for m in c.mis) == [1, 2, 3, 5, 8, 15] == sorted(m for c in mis if c.in_dt == "u8hwc" for m in c.mis)
    assert all(sorted(c.mis) == [2, 6, 14] for c in mis if c.in_dt in ("f16", "bf16")) and {c.in_dt for c in mis} == {"u8", "u8hwc", "f16", "bf16", "f32"}
    assert [sorted(c.mis) for c in mis if c.in_dt == "f32"] == [[4, 12]]
    for case in mis:
        (kind, rpw, cg), = _tiled(case)
        tiles = P.lb_tiles(case, rpw, cg)
        for i in range(len(case.geoms)):
            mine = [t for t in tiles if t["img"] == i]
            assert mine and any(t["al_a"] != 0 for t in mine), (case.name, i)
            assert all(t["al_r"] != 0 for t in mine) and (case.in_dt == "u8hwc" or all(t["al_p"] != 0 for t in mine)), (case.name, i)


def test_single_column_cases_have_a_tile_of_span_one():
    for name in ("cpr1-a", "cpr1-b", "cpr1-c", "one-win"):
        case = P.LB_BY_NAME[name]
        for _, knob, cg in P.LB_VARIANTS:
            for d in P.lb_dispatch(case, knob, cg):
                if d[0] == "tile" and (d[2] == 1 or name == "one-win"):
                    assert any(t["span"] == 1 for t in P.lb_tiles(case, d[1], d[2])), (name, d)


def test_fallback_case_exceeds_the_lds_request_at_one_row_per_wave():
    case = P.LB_BY_NAME["fallback-f32"]
    assert P.lb_tile_lds(case, case.geoms, 4, P.LB_TW) == 0 and P.lb_tile_lds(case, case.geoms[:1], 16, P.LB_TW) > 0   # the batch does not fit; its first image alone does
    hin, win, hr, wr, _, _ = case.geoms[1]
    assert 3 * min(int(4 * (hin / hr)) + 3, hin) * (((min(int(128 * (win / wr)) + 3, win) * 4 + 30) >> 4) << 4) > 64 * 1024
    assert all(P.lb_dispatch(case, knob, cg) == [("pixel",)] for _, knob, cg in P.LB_VARIANTS)
    for name in ("down3-bf16", "down3-u8hwc"):
        assert P.lb_dispatch(P.LB_BY_NAME[name])[0][0] == "tile"
    assert P.lb_dispatch(P.LB_BY_NAME["n66-f16"]) == [("tile", 4, 1)] * 2


# ---- 1. letterbox: the kernels on the simulator ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LB_NAMES)
def test_letterbox_equals_the_model_bit_for_bit(lib, name):
    case = P.LB_BY_NAME[name]
    # the 66-image cases run the default and one forced variant of each kernel here (the simulator takes half a second per variant); the GPU file runs them all
    few = name.startswith("n66")
    outs = P.check_letterbox(lib, case, variants=[v for v in P.LB_VARIANTS if v[0] in ("default", "pixel-cg1", "1-cg2")] if few else P.LB_VARIANTS)
    if name.startswith("n66"):
        assert torch.equal(P.bits(outs["default"][63:]), P.bits(P.lb_model(case)[63:])) and len(case.geoms) == 66


# ---- 2. SPP pyramid --------------------------------------------------------------------------------------------------------------------------------------------------
def test_spp_threshold_pairs_lie_on_either_side_of_the_lds_budget():
    assert [P.spp_fit(g) for g in (4, 2, 1)] == [1276, 2552, 5104]
    for fit, miss, g in P.SPP_THRESHOLD_PAIRS:
        a, b = P.SPP_BY_NAME[fit], P.SPP_BY_NAME[miss]
        assert a.h * a.w == P.spp_fit(g) and b.h * b.w > P.spp_fit(g) and a.h * a.w * g * P.SPP_BLOCK_BYTES <= P.SPP_LDS < b.h * b.w * g * P.SPP_BLOCK_BYTES
        assert P.spp_path(a, "f16") == ("lds", g) and P.spp_path(b, "f16") == (("lds", g // 2) if g > 1 else ("direct",))
    assert P.spp_path(P.SPP_BY_NAME["fit-g1"], "f32") == ("lds32",) and P.spp_path(P.SPP_BY_NAME["direct"], "f32") == ("direct32",)
    assert {c.c: P.spp_path(c, "bf16")[1] for c in P.SPP_CASES if c.name.startswith("auto")} == {32: 4, 16: 2, 48: 2, 8: 1, 24: 1, 40: 1}
    assert [P.spp_path(P.SPP_BY_NAME[f"force-g{g}"], "f16") for g in (1, 2, 4)] == [("lds", 1), ("lds", 2), ("lds", 4)]


def test_spp_inputs_hold_the_values_the_issue_lists():
    x = P.spp_input("f16", 3, 8, 20, 17)
    b = P.bits(x)
    sub = ((b & 0x7c00) == 0) & ((b & 0x03ff) != 0)
    for pattern in (0x0001, -0x7fff, 0x7bff, -0x0401, 0x7c00, -0x0400, 0x0000, -0x8000):   # +-2^-24, +-65504, +-inf, +-0 (int16 views)
        assert (b == pattern).any(), hex(pattern & 0xffff)
    assert (sub & (b > 0)).any() and (sub & (b < 0)).any() and float(sub.float().mean()) > 0.1
    assert (x[:, 1].float() < 0).all() and all(len(torch.unique(x[i, 2])) == 1 for i in range(3))
    assert float(x[0, 3].float().max()) == float(x[0, 3, 0, 0]) == 65504.0 and torch.isinf(x[1, 3, -1, -1])
    for dt in ("bf16", "f32"):
        y = P.spp_input(dt, 3, 8, 20, 17).float()
        assert torch.isinf(y).any() and ((y != 0) & (y.abs() < 2.0 ** -126)).any() and (y.abs() > 1e30).any() and not torch.isnan(y).any()


@pytest.mark.parametrize("name", [c.name for c in P.SPP_CASES if not c.name.startswith("nt-")])
def test_spp_pyramid_is_exact(lib, name):
    case = P.SPP_BY_NAME[name]
    for dt in case.dts:
        P.check_spp(lib, case, dt)


def test_spp_results_do_not_depend_on_the_block_size(lib):
    for dt in ("f16", "bf16"):
        runs = [P.check_spp(lib, P.SPP_BY_NAME[f"nt-{nt}"], dt) for nt in (256, 512, 1024)]
        for other in runs[1:]:
            assert all(torch.equal(P.bits(a), P.bits(b)) for a, b in zip(runs[0], other))


# ---- 3. upsample and view copy, 4. layout ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("hw", P.UP_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_upsample_and_view_copy_move_raw_bits(lib, dt, hw):
    P.check_upsample_and_copy(lib, dt, *hw)


def test_raw_patterns_hold_nan_patterns():
    assert torch.isnan(P.raw_patterns("f16", (4096,), 1).view(torch.float16)).any() and torch.isnan(P.raw_patterns("f32", (4096,), 1).view(torch.float32)).any()


@pytest.mark.parametrize("pair", P.LAYOUT_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
@pytest.mark.parametrize("hw", P.LAYOUT_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_layout_conversion_rounds_to_nearest_even(lib, pair, hw):
    P.check_layout(lib, pair[0], pair[1], *hw)


def test_layout_values_hold_ties_overflow_and_subnormal_results():
    x = P.layout_values("f32", (2, 3, 7, 9), seed=0)
    h, b = x.to(torch.float16), x.to(torch.bfloat16)
    assert torch.isinf(h).any() and torch.isinf(b).any() and not torch.isinf(x).any()
    assert ((h.float() != 0) & (h.float().abs() < 2.0 ** -14)).any() and ((b.float() != 0) & (b.float().abs() < 2.0 ** -126)).any()
    assert (P.bits(x) == -2 ** 31).any()                                                      # -0
    for v, lo, hi in ((1 + 2.0 ** -11, 1.0, None), (1 + 3 * 2.0 ** -11, None, 1 + 2.0 ** -9)):   # exact fp16 ties: kept mantissa even (down) and odd (up)
        assert (x == v).any() and float(torch.tensor(v).half()) == (lo if lo is not None else hi)
    for v, want in ((1 + 2.0 ** -8, 1.0), (1 + 3 * 2.0 ** -8, 1 + 2.0 ** -6)):                   # exact bf16 ties
        assert (x == v).any() and float(torch.tensor(v).bfloat16()) == want


def test_layout_empty_batch_and_refused_pairs(lib):
    P.check_layout_edges(lib)
