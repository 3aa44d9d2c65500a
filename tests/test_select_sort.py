"""CPU side of tests/test_select_sort_gpu.py: every case of tests/_select_cases.py is shown, from the oracle alone, to say something about the score-prefix
selection and the per-image sorts (postprocess.hip) -- and the constants the cases are built around are the ones the kernels use."""
import os
import re

import pytest

import _select_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source():
    with open(os.path.join(ROOT, "yolort_amd", "csrc", "postprocess.hip")) as f:
        return f.read()


@pytest.mark.parametrize("name", ["RANK_MAX", "SEL_SLICE", "SEL_BINS", "IMG_SORT_MAX"])
def test_constants_match_the_kernels(name):
    """a changed constant fails here, by name, instead of quietly moving the cases off the edges they were built for"""
    m = re.findall(r"constexpr int %s = (\d+);" % name, _source())
    assert m == [str(getattr(S, name))], (name, m)


def test_sel_t_rule_matches_the_host():
    """sel_t = max(4 * detections_per_img, 4096), an image is cut when it holds more than 1.5 * sel_t records, the LDS run of sort_image_kernel is IMG_SORT_MAX
    under YMI_POST_EXACT_FULL and half of it otherwise, the multi-block form needs two slices and fewer than 32 images"""
    src = _source()
    assert "const int sel_t = exact_full ? 0 : (4 * d->detections_per_img > 4096 ? 4 * d->detections_per_img : 4096);" in src
    assert src.count("n_i <= sel_t + sel_t / 2") == 2    # sel_hist_kernel and select_prefix_kernel
    assert "const int run_max = exact_full ? IMG_SORT_MAX : IMG_SORT_MAX / 2;" in src
    assert "cap_img >= 2 * SEL_SLICE && d->n < multi_max_n" in src and ': 32;   // tuning aid' in src
    assert [S.sel_t(k) for k in S.K_SWEEP] == [4096, 6000, 6144, 6148, 8000, 8192, 8196, 12000]
    assert not S.is_cut(6144, 300) and S.is_cut(6145, 300)


@pytest.mark.parametrize("case", S.ALL_CASES, ids=repr)
def test_case_conditions(case):
    """the exact record counts, the minimum-gap rule (unequal scores >= 1e-5 relative apart under the oracle's decode), fat / plain crossing bins, and the condition of
    the case's kind: "suffices" -- at least k survivors within the top sel_t records and the last returned one beyond rank sel_t / 2; "short" -- fewer than k survivors
    within the top max(RANK_MAX, sel_t).  Prints the candidate count, both survivor counts and the rank of the last returned survivor of every image."""
    if case.exact:   # no selection: the counts and the gap rule only
        st = S.stats(case.data, case.k, case.agnostic)
        for i, (s, r) in enumerate(zip(st, S.reference(case.data, case.agnostic))):
            print(f"{case} image {i}: candidates {s['count']} survivors {s['survivors']} last returned survivor at rank {s['last_rank']}")
            assert s["count"] == case.data.counts[i] and S.min_relative_gap(r["all_scores"]) >= S.MIN_GAP
            assert s["survivors"] > 0
        return
    st = S.assert_case(case.data, case.k, case.kind, case.agnostic)
    assert [S.is_cut(s["count"], case.k) for s in st] == case.cut()


def test_patterns_and_counts_are_all_there():
    """every score pattern is cut at least once, and the crowded images hold the record counts around the edges: 6144 / 6145 (1.5 * sel_t), 16384 / 16385 (a slice,
    an LDS run), the whole map at 4 and at 8 classes"""
    cut_patterns = {p for c in S.ALL_CASES for (p, n), cut in zip(c.data.images, c.cut()) if cut}
    assert cut_patterns == set(S.PATTERNS) - {"sparse"}
    counts = {n for c in S.ALL_CASES for _, n in c.data.images}
    assert {6144, 6145, 16384, 16385, 4 * S.ANCHORS_PER_IMAGE, 8 * S.ANCHORS_PER_IMAGE} <= counts
    assert 8 * S.ANCHORS_PER_IMAGE > 3 * S.SEL_SLICE and 8 * S.ANCHORS_PER_IMAGE % S.SEL_SLICE != 0    # four slices, the last one ragged
