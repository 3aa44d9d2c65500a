"""The letterbox, SPP, upsample, view-copy and layout kernels of csrc/preproc_pool.hip on the GPU: the cases of tests/_pre_cases.py (the same ones
tests/test_pre_exact.py runs on the simulator) on the real kernels, through the same drivers -- poisoned destinations between guard bands, every comparison on raw bits.
Yardsticks, case tables and the kernel-to-case table: tests/_pre_cases.py."""
import pytest
import torch

import _pre_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from yolort_amd import _lib
    return P.proto(_lib.load(require_gpu=True))


# ---- 1. letterbox ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in P.LB_CASES])
def test_letterbox_equals_the_model_bit_for_bit(dev, lib, name):
    """every kernel variant (YOLORT_AMD_LETTERBOX = pixel / 1 / 2 / 4, each with YOLORT_AMD_LB_CG 1 and 2, and the default) equals the NumPy model bit for bit"""
    case = P.LB_BY_NAME[name]
    outs = P.check_letterbox(lib, case, dev)
    assert set(outs) == {v[0] for v in P.LB_VARIANTS}
    if name.startswith("n66"):   # the second launch (images 64 and 65) and the last image of the first land where the model puts them
        for got in outs.values():
            assert torch.equal(P.bits(got[63:]), P.bits(P.lb_model(case)[63:])) and len(case.geoms) == 66


# ---- 2. SPP pyramid ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in P.SPP_CASES if not c.name.startswith("nt-")])
def test_spp_pyramid_is_exact(dev, lib, name):
    case = P.SPP_BY_NAME[name]
    for dt in case.dts:
        P.check_spp(lib, case, dt, dev)


def test_spp_results_do_not_depend_on_the_block_size(dev, lib):
    for dt in ("f16", "bf16"):
        runs = [P.check_spp(lib, P.SPP_BY_NAME[f"nt-{nt}"], dt, dev) for nt in (256, 512, 1024)]
        for other in runs[1:]:
            assert all(torch.equal(P.bits(a), P.bits(b)) for a, b in zip(runs[0], other))


# ---- 3. upsample and view copy, 4. layout ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("hw", P.UP_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_upsample_and_view_copy_move_raw_bits(dev, lib, dt, hw):
    P.check_upsample_and_copy(lib, dt, *hw, device=dev)


@pytest.mark.parametrize("pair", P.LAYOUT_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
@pytest.mark.parametrize("hw", P.LAYOUT_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_layout_conversion_rounds_to_nearest_even(dev, lib, pair, hw):
    P.check_layout(lib, pair[0], pair[1], *hw, device=dev)


def test_layout_empty_batch_and_refused_pairs(dev, lib):
    P.check_layout_edges(lib, dev)
