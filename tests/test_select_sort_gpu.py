"""The per-image score-prefix selection and the two per-image sorts of the post-process (postprocess.hip) on the GPU, path by path: select_prefix_kernel alone
(YOLORT_AMD_SEL_SINGLE=1, regions of 16384 records, a batch of 32), the multi-block form (sel_hist / the sel_rhist + sel_rpick ladder / sel_compact / sel_copyback
over two and four slices), the ranking sort and sort_image_kernel with one to four runs.  Inputs and their conditions: tests/_select_cases.py (asserted from the
oracle alone by tests/test_select_sort.py).  Every run goes through Plan.postprocess with a chosen capacity and flags, outputs pre-filled; the status words are
read after ONE pass, then the host protocol of yolort_amd/ops.py is followed to the end.

Asserted per run: counts, labels and order equal the oracle's post-process of the FULL candidate set, scores / boxes to the rounding of expf, nothing written past
the counts; status[4] is the oracle's candidate count, no overflow bit, YMI_STATUS_PREFIX_SHORT exactly in the "short" cases; the selection size S of the cut
images (status[0] minus the records of the images that must not be cut) lies in [sel_t, max(RANK_MAX, sel_t)]."""
import numpy as np
import pytest
import torch

import _select_cases as S

pytestmark = pytest.mark.gpu
FILL = -3.0
SINGLE_ENV = "YOLORT_AMD_SEL_SINGLE"   # read by the library at every call


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


def _inputs(dev, data):
    """the batch's head output in the layout the op reads: (n, h, w, 3 * (nc + 5) padded to a multiple of 4)"""
    ho = data.heads()[0]
    n, kk = ho.shape[0], data.nc + 5
    cs = (3 * kk + 3) // 4 * 4
    t = torch.zeros(n, S.H, S.W, cs, device=dev, dtype=torch.float32)
    t[..., : 3 * kk] = ho.to(dev).permute(0, 2, 3, 1, 4).reshape(n, S.H, S.W, 3 * kk)
    return t


def _plan(dev, t, data, k, cap_img, flags):
    from yolort_amd.engine import Plan, View
    n = t.shape[0]
    plan = Plan(dev, torch.float16)
    view = View(t.view(-1), 0, n, S.H, S.W, 3 * (data.nc + 5), t.shape[3])
    pb = plan.postprocess([view], data.strides, data.anchors, data.nc, S.THR, S.NMS_THR, k, n * cap_img, flags=flags)
    return plan, pb


def _run_plan(plan, pb):
    """one pass with pre-filled outputs -> (status words, outputs on the host)"""
    pb.boxes.fill_(FILL), pb.scores.fill_(FILL), pb.labels.fill_(int(FILL)), pb.status_count.fill_(int(FILL))
    plan.run()
    torch.cuda.synchronize()
    return pb.status.cpu().tolist(), dict(count=pb.count.cpu(), labels=pb.labels.cpu(), scores=pb.scores.cpu(), boxes=pb.boxes.cpu())


def _flags(case):
    from yolort_amd import _lib
    return (_lib.POST_AGNOSTIC if case.agnostic else 0) | (_lib.POST_EXACT_FULL if case.exact else 0)


_RUNS = {}


def _run(dev, case, cap_img, single):
    """first-pass status and final outputs of a case on one path; kept per (case, path), so that a test that compares two paths does not run either twice"""
    from yolort_amd import _lib
    key = (case.name, cap_img, single)
    if key in _RUNS:
        return _RUNS[key]
    t = _inputs(dev, case.data)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv(SINGLE_ENV, "1") if single else mp.delenv(SINGLE_ENV, raising=False)
        plan, pb = _plan(dev, t, case.data, case.k, cap_img, _flags(case))
        first, out = _run_plan(plan, pb)
        last = first
        if first[1] == 2:   # YMI_STATUS_PREFIX_SHORT alone: the exact full pass follows (an overflow is a failure of the test, not something to recover from)
            plan, pb = _plan(dev, t, case.data, case.k, cap_img, _flags(case) | _lib.POST_EXACT_FULL)
            last, out = _run_plan(plan, pb)
    _RUNS[key] = dict(first=first, last=last, out=out)
    return _RUNS[key]


def _assert_equals_oracle(out, ref):
    """counts, labels, order exact; scores / boxes to the rounding of expf (the constants of test_ops_gpu.py::_assert_post_equals_oracle); nothing written past the counts"""
    for i, r in enumerate(ref):
        c = int(out["count"][i])
        assert c == len(r["scores"]), (i, c, len(r["scores"]))
        np.testing.assert_array_equal(out["labels"][i, :c].numpy(), r["labels"].numpy(), err_msg=f"image {i}")
        np.testing.assert_allclose(out["scores"][i, :c].numpy(), r["scores"].numpy(), rtol=2e-6, atol=1e-7, err_msg=f"image {i}")
        np.testing.assert_allclose(out["boxes"][i, :c].numpy(), r["boxes"].numpy(), rtol=1e-5, atol=1e-4, err_msg=f"image {i}")
        assert (out["scores"][i, c:] == FILL).all() and (out["labels"][i, c:] == int(FILL)).all() and (out["boxes"][i, c:] == FILL).all(), f"image {i}: slots past the count were written"


def _check(dev, case, cap_img, single=False):
    run = _run(dev, case, cap_img, single)
    first, last = run["first"], run["last"]
    counts, cut = case.data.counts, case.cut()
    t, hi = S.sel_t(case.k), max(S.RANK_MAX, S.sel_t(case.k))
    selected = first[0] - sum(c for c, x in zip(counts, cut) if not x)
    print(f"{case} cap_img={cap_img} single={single}: first pass {first}, selected {selected} records in {sum(cut)} cut image(s), sel_t={t}")
    assert max(counts) <= cap_img, "the case does not fit the regions"
    assert first[4] == sum(counts), f"raw candidates {first[4]}, the oracle has {sum(counts)}"
    assert not first[1] & 1, f"overflow reported: {first}"
    assert bool(first[1] & 2) == (case.kind == "short"), f"YMI_STATUS_PREFIX_SHORT: {first}, case kind {case.kind}"
    assert sum(cut) * t <= selected <= sum(cut) * hi, f"selection size {selected} outside [{t}, {hi}] per cut image"
    assert last[1] == 0 and last[4] == sum(counts), last
    _assert_equals_oracle(run["out"], S.top_k(S.reference(case.data, case.agnostic), case.k))
    return run


def _assert_same(a, b):
    assert a["first"][0] == b["first"][0] and a["first"][1] == b["first"][1], (a["first"], b["first"])
    for key in ("count", "labels", "scores", "boxes"):
        assert torch.equal(a["out"][key], b["out"][key]), f"{key} differ between the two forms"


def _cap_for(case):
    return 65536 if max(case.data.counts) > 32768 else 32768


@pytest.mark.parametrize("case", S.PATTERN_CASES, ids=repr)
def test_multi_block_selection(dev, case):
    """every score pattern through the multi-block form (two images: n < 32; regions of 32768 records = two slices, 65536 = four, the last one ragged for the whole
    nc = 8 map): a plain cut, a fat bin refined by the ladder, all-equal scores down to the candidate-id bits, a cut inside the ties of the lower of two values,
    bin 0 together with the last bin; the crowded image is followed by a sparse one that must be left alone.

    all-equal, two-valued, top-and-bottom and the 6145-record fat bin put the crossing bin LAST among the populated ones.  Before this test such an image was
    "nothing to cut" and went whole (up to 27648 records here) to sort_image_kernel, in both forms: right detections, selection size = record count, never
    YMI_STATUS_PREFIX_SHORT.  It is refined like any other fat bin now."""
    _check(dev, case, _cap_for(case))


@pytest.mark.parametrize("case", S.PATTERN_CASES, ids=repr)
def test_one_block_selection_by_switch_agrees(dev, case):
    """the same cases with YOLORT_AMD_SEL_SINGLE=1: select_prefix_kernel streams, refines and compacts the image alone -- and returns bit for bit what the multi-block
    form returned, with the same number of selected records (the ladder restates the one-block refinement's arithmetic)"""
    cap = _cap_for(case)
    _assert_same(_check(dev, case, cap, single=True), _check(dev, case, cap))


@pytest.mark.parametrize("case", [c for c in S.PATTERN_CASES if max(c.data.counts) <= 16384], ids=repr)
def test_one_block_selection_by_small_regions(dev, case):
    """regions of 16384 records (one slice): the one-block form without the switch; an image of exactly 16384 records fills its region"""
    _check(dev, case, 16384)


def test_one_block_selection_in_a_batch_of_32(dev):
    """32 images take the one-block form by default: images 0 and 31 crowded (a fat bin; all-equal scores), thirty sparse ones between them -- the compact offsets
    of the sorts run across all 32"""
    _check(dev, S.BATCH32, 32768)


def test_cut_sparse_and_uncut_images_in_one_batch(dev):
    """image 0 is cut, image 1 is sparse, image 2 holds exactly 1.5 * sel_t records (crowded, not cut); both forms, bit-identical"""
    _assert_same(_check(dev, S.MIXED3, 32768), _check(dev, S.MIXED3, 32768, single=True))


@pytest.mark.parametrize("case", S.K_CASES + [S.K_SHORT, S.K_EQUAL_IMAGES], ids=repr)
def test_detections_per_img_sweep(dev, case):
    """sel_t = 4096, 6000, 6144, then past RANK_MAX: 6148, 8000, 8192 (the cut image takes ONE run of sort_image_kernel), 8196 and 12000 (two runs).  Past RANK_MAX
    the ladder walks to the exhausted key and selects exactly sel_t records, all of which sel_copyback_kernel has to bring back.  Multi-block form (four slices)
    and one-block form, bit-identical.

    sel_t = 6148 is four records past RANK_MAX; the last case runs it on six equal crowded images, which lose or keep their records independently.

    On the commit before this test, detections_per_img >= 1537 failed in the multi-block form only: sel_copyback_kernel copied RANK_MAX records per image at most
    (wrong labels in 12 % of the slots at 1537, 87 % from 2000 on, YMI_STATUS_PREFIX_SHORT at 3000; no status bit otherwise)."""
    _assert_same(_check(dev, case, 65536), _check(dev, case, 65536, single=True))
    if S.sel_t(case.k) > S.RANK_MAX:
        assert _run(dev, case, 65536, False)["first"][0] == sum(case.cut()) * S.sel_t(case.k) + S.SPARSE[1], "past RANK_MAX the selection is exact"


@pytest.mark.parametrize("case", S.EXACT_CASES + S.EXACT_MIXED, ids=repr)
def test_exact_full_sorts(dev, case):
    """YMI_POST_EXACT_FULL from the first pass (no selection): 6144 records take the ranking sort, 6145 one LDS run of sort_image_kernel, 16384 one full run, 16385 two,
    55296 four with a ragged last one; the two mixed batches put a ranking-sort image before / behind a two-run image -- both kernels write one compact array"""
    run = _check(dev, case, _cap_for(case))
    assert run["first"][0] == sum(case.data.counts)


@pytest.mark.parametrize("case", S.AGNOSTIC_CASES, ids=repr)
def test_agnostic_selection_and_sorts(dev, case):
    """YMI_POST_AGNOSTIC (P keys without label bits) on a fat bin and on a cut image that takes two runs of sort_image_kernel; both selection forms, bit-identical"""
    _assert_same(_check(dev, case, 65536), _check(dev, case, 65536, single=True))


@pytest.mark.parametrize("case,other", [(S.CASES["all-equal-27648-aw80-k300"], S.CASES["fat-bin-16385-aw110-k300"]),
                                        (S.CASES["fat-bin-55296-aw158-k300"], S.CASES["spread-55296-aw48-k2000"]),
                                        (S.CASES["spread-55296-aw48-k2000"], S.CASES["fat-bin-55296-aw158-k300"])], ids=repr)
def test_used_workspace(dev, case, other):
    """the plan of `case` runs, then runs again on the workspace another batch (other data, same shapes) left behind: identical outputs and status words.  Nothing may
    rely on zeroed or on its own stale scratch -- the ladder's histograms, the fill counters and the per-image states are where that would show."""
    cap = _cap_for(case)
    assert other.data.nc == case.data.nc and other.data.n == case.data.n
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv(SINGLE_ENV, raising=False)
        t, t_o = _inputs(dev, case.data), _inputs(dev, other.data)   # (the plans read them at every run: both stay alive)
        plan, pb = _plan(dev, t, case.data, case.k, cap, _flags(case))
        plan_o, pb_o = _plan(dev, t_o, other.data, case.k, cap, _flags(case))
        assert pb.ws.numel() == pb_o.ws.numel()
        first, out = _run_plan(plan, pb)
        _run_plan(plan_o, pb_o)
        pb.ws.copy_(pb_o.ws)
        again, out2 = _run_plan(plan, pb)
    assert first[1] == 0 and again == first, (first, again)
    for key in out:
        assert torch.equal(out[key], out2[key]), f"{key} differ on a used workspace"
    _assert_equals_oracle(out2, S.top_k(S.reference(case.data), case.k))
