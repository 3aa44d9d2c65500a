"""NV12 drawing and cropping without a GPU: the integer RGB -> YCbCr contract (include/yolort_amd.h) against the real-valued formula, the cases' own claims, and
render_nv12_kernel with its host routing on the CPU simulator -- the simulator library of tests/test_nv12.py is csrc/preproc_nv12.hip as a whole, so it holds the new
kernels without a new translation unit.  Yardsticks and cases: tests/_nv12draw_cases.py; the GPU twin is tests/test_nv12_draw_gpu.py."""
import numpy as np
import pytest

import _nv12draw_cases as D
from _nv12_cases import TABLES
from test_nv12 import sim  # noqa: F401  (the module-scoped fixture that builds the simulator library of csrc/preproc_nv12.hip)


@pytest.mark.parametrize("matrix,full", TABLES)
def test_integer_contract_is_within_the_derived_bound_of_the_real_formula(matrix, full):
    """every RGB triple of a grid with 0, 1, 127, 128, 254, 255 per channel and a seeded random sample; the header's 36 integers are the rounded real coefficients"""
    grid = np.unique(np.r_[0, 1, 127, 128, 254, 255, np.arange(5, 255, 9)])
    rgb = np.concatenate([np.stack(np.meshgrid(grid, grid, grid, indexing="ij"), -1).reshape(-1, 3), np.random.default_rng(1).integers(0, 256, (20000, 3))])
    real = D.ycc_real(rgb, matrix, full)
    err = np.abs(D.ycc_int(rgb, matrix, full, clamp=False) - real).max()   # before the clamp (full-range chroma of a saturated channel is 255.5)
    print(f"{matrix} full={full}: max |codes - real formula| = {err:.5f}, bound {D.YCC_BOUND:.5f}")
    assert err <= D.YCC_BOUND
    unit = D.ycc_real(np.eye(3) * 16384, matrix, full) - D.ycc_real(np.zeros((1, 3)), matrix, full)   # column j = the nine real coefficients x 2^14
    assert np.array_equal(np.rint(unit.T.reshape(-1)), D._lib.YCC_COEF[(matrix, full)])
    header = open(D.T.ROOT + "/include/yolort_amd.h").read().replace(" ", "")
    assert "{" + ",".join(str(v) for v in D._lib.YCC_COEF[(matrix, full)]) + "}" in header and "0.5+3*255*2^-15" in header


def test_cases_exercise_what_they_are_about():
    D.check_claims()


@pytest.mark.parametrize("name", list(D.CASES))
def test_render_nv12_on_the_simulator_equals_the_painter_bit_for_bit(sim, name):  # noqa: F811
    D.check(sim, D.CASES[name])


def test_refusals_on_the_simulator(sim):  # noqa: F811
    D.check_refusals(sim)
