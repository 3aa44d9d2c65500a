"""On-device COCO matching on the MI355X: eval_match_kernel through ops.match_detections / ymi_eval_match on the synthetic slabs of tests/_eval_cases.py -- every flag, rank
and ground-truth count exact against the host oracle (the matching loop of metrics.coco_ap restated in _eval_cases.match_one), nothing written outside the defined slots --
and metrics.GpuDetectionEvaluator against the unchanged DetectionEvaluator: the dicts are EQUAL, not close.  No model, no plan."""
import numpy as np
import pytest
import torch

import _eval_cases as E
from yolort_amd.utils import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(case):
    return [torch.from_numpy(case[k]).to(DEV) for k in ("boxes", "scores", "labels", "counts", "gt_boxes", "gt_labels", "gt_counts")]


def _run(case, out=None):
    """one launch on outputs prefilled with the sentinels -> the outputs as numpy (tp / ig as uint16)"""
    from yolort_amd import ops
    N, K = case["scores"].shape
    R = len(case["rngs"])
    if out is None:
        out = dict(tp=torch.full((R, N, K), E.SENT16, dtype=torch.int16, device=DEV), ig=torch.full((R, N, K), E.SENT16, dtype=torch.int16, device=DEV),
                   rank=torch.full((N, K), E.SENT_RANK, dtype=torch.int32, device=DEV), n_gt=torch.full((R, case["C"]), E.SENT_NGT, dtype=torch.int32, device=DEV),
                   status=torch.zeros(4, dtype=torch.int32, device=DEV))
    ops._launch_eval_match(*_dev(case), case["C"], case["thrs"], case["rngs"], case["max_dets"], **out)
    return out, {k: (v.cpu().numpy().view(np.uint16) if v.dtype == torch.int16 else v.cpu().numpy()) for k, v in out.items()}


CASES = {
    **{f"lane wrap {n}": (lambda n=n: E.lane_wrap_case(n)) for n in E.LANE_WRAP},
    "counts max_dets 100": lambda: E.det_counts_case(100),
    "counts max_dets 2": lambda: E.det_counts_case(2),
    "counts no cut": lambda: E.det_counts_case(None),
    "score order": E.score_order_case,
    "iou boundaries": E.iou_boundary_case,
    "iou tie": E.iou_tie_case,
    "greedy": E.greedy_case,
    "area ranges": E.area_case,
    "degenerate": E.degenerate_case,
    "one image": lambda: E.random_case(8, n_img=1, n_det=40, n_gt=6, C=4),
    "33 ragged images": lambda: E.random_case(9, n_img=33, n_det=12, n_gt=5, C=4, ragged=True),
    # the limits (more than 64 KiB of LDS: the large-LDS launch), 16 positions per lane, the thresholds 0.5 and 1.0
    "1024 x 1024": lambda: E.random_case(10, n_img=1, n_det=1024, n_gt=1024, C=8, max_dets=None, thrs=[0.5, 1.0], rngs=(E.INF_RNG, M.COCO_AREA_RNG["medium"])),
    "nan score": E.nan_score_case,
    "bad label": E.bad_label_case,
    "stale row": E.stale_case,
}


@pytest.mark.parametrize("name", list(CASES))
def test_eval_match_vs_oracle(name):
    case = CASES[name]()
    E.assert_outputs(case, _run(case)[1])


def test_match_detections_returns_the_flags_and_raises_on_status():
    from yolort_amd import ops
    case = E.random_case(12, n_img=3, n_det=20, n_gt=5, C=4, max_dets=7, thrs=[0.5, 0.9], rngs=(M.COCO_AREA_RNG["small"],))
    tp, ig, rank, n_gt = ops.match_detections(*_dev(case), case["C"], case["thrs"], case["rngs"], case["max_dets"])
    exp = E.expected(case)
    live = exp["rank"] != E.SENT_RANK
    np.testing.assert_array_equal(tp.cpu().numpy().view(np.uint16)[0][live], exp["tp"][0][live])
    np.testing.assert_array_equal(ig.cpu().numpy().view(np.uint16)[0][live], exp["ig"][0][live])
    np.testing.assert_array_equal(rank.cpu().numpy()[live], exp["rank"][live])
    np.testing.assert_array_equal(n_gt.cpu().numpy(), exp["n_gt"] - E.SENT_NGT)
    # the defaults: COCO's ten thresholds, one range that ignores nothing, no cut
    tp, ig, rank, n_gt = ops.match_detections(*_dev(case), case["C"])
    case_d = dict(case, thrs=[float(t) for t in M.COCO_IOU_THRS], rngs=(E.INF_RNG,), max_dets=None)
    exp = E.expected(case_d)
    np.testing.assert_array_equal(tp.cpu().numpy().view(np.uint16)[0][live], exp["tp"][0][live])
    np.testing.assert_array_equal(rank.cpu().numpy()[live], exp["rank"][live])
    for bad, msg in ((E.bad_label_case(), "outside"), (E.stale_case(), "stale shard")):
        with pytest.raises(ValueError, match=msg):
            ops.match_detections(*_dev(bad), bad["C"])


REFUSALS = [("k", dict(K=1025)), ("g", dict(G=1025)), ("thresholds", dict(thrs=[0.5] * 17)), ("ranges", dict(rngs=[E.INF_RNG] * 5)), ("zero threshold", dict(thrs=[0.5, 0.0]))]


@pytest.mark.parametrize("what,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, kw):
    from yolort_amd import ops
    from yolort_amd._lib import YmiError
    base = dict(K=None, G=None, thrs=None, rngs=E.COCO_RNGS)
    base.update(kw)
    case = E.make_case([(np.zeros((1, 4)), np.ones(1, np.float32), np.zeros(1, np.int64))], [(np.zeros((1, 4)), np.zeros(1, np.int32))], C=2, poison=False, **base)
    with pytest.raises(YmiError, match="code -1"):
        ops.match_detections(*_dev(case), case["C"], case["thrs"], case["rngs"], case["max_dets"])


def test_cpu_tensors_are_refused():
    from yolort_amd import ops
    from yolort_amd._lib import YmiError
    case = E.greedy_case()
    args = _dev(case)
    args[4] = args[4].cpu()
    with pytest.raises(YmiError):
        ops.match_detections(*args, case["C"])


# ---- the evaluator -------------------------------------------------------------------------------------------------------------------------------------------------
def _host_dict(cases, num_classes, max_dets):
    ev = M.DetectionEvaluator(num_classes, max_dets)
    for case in cases:
        ev.update(*E.to_lists(case))
    return ev.compute()


def _slab_and_targets(case):
    b, s, l, c, gb, gl, gc = _dev(case)
    return (b, s, l, c), (gb, gl, gc)


@pytest.fixture(scope="module")
def round_trip():
    """the random round-trip cases and the host evaluator's dicts, computed once"""
    cases = [E.random_case(seed, n_img=6, n_det=300, n_gt=8, C=80) for seed in E.RANDOM_SEEDS]
    return cases, [_host_dict([c], 80, M.COCO_MAX_DETS) for c in cases], _host_dict(cases, 80, M.COCO_MAX_DETS)


def test_evaluator_equals_the_host_evaluator(round_trip):
    cases, singles, _ = round_trip
    for case, want in zip(cases, singles):
        ev = M.GpuDetectionEvaluator(80)
        ev.update_from_slab(*_slab_and_targets(case))
        got = ev.compute()
        print(got)
        assert got == want and all(v > 0 for v in want.values())


def test_two_updates_and_merge_equal_one_evaluator(round_trip):
    cases, _, both = round_trip
    ev = M.GpuDetectionEvaluator(80)
    for case in cases:
        ev.update_from_slab(*_slab_and_targets(case))
    assert ev.compute() == both
    whole = {k: (np.concatenate([c[k] for c in cases]) if isinstance(cases[0][k], np.ndarray) else cases[0][k]) for k in cases[0]}
    one = M.GpuDetectionEvaluator(80)
    one.update_from_slab(*_slab_and_targets(whole))
    assert one.compute() == both and torch.equal(one._n_gt, ev._n_gt)
    a, b = M.GpuDetectionEvaluator(80), M.GpuDetectionEvaluator(80)
    a.update_from_slab(*_slab_and_targets(cases[0]))
    b.update_from_slab(*_slab_and_targets(cases[1]))
    a.merge(b)
    assert a.compute() == both and torch.equal(a._n_gt, one._n_gt)


def test_update_from_lists_small_classes_and_no_cut():
    """update() pads the lists (device detections, host targets) into slabs; ragged counts, empty images, max_dets None and 2; classes without ground truth or
    without detections"""
    case = E.random_case(9, n_img=33, n_det=12, n_gt=5, C=4, ragged=True)
    preds, targets = E.to_lists(case)
    for max_dets in (None, 2):
        ev = M.GpuDetectionEvaluator(4, max_dets)
        ev.update([{k: torch.from_numpy(v).to(DEV) for k, v in p.items()} for p in preds], [{k: torch.from_numpy(v) for k, v in t.items()} for t in targets])
        assert ev.compute() == _host_dict([case], 4, max_dets)
    special = [E.area_case(), E.degenerate_case(), E.iou_boundary_case(), E.score_order_case(), E.nan_score_case()]
    for case in special:
        ev = M.GpuDetectionEvaluator(case["C"])
        ev.update_from_slab(*_slab_and_targets(case))
        assert ev.compute() == _host_dict([case], case["C"], M.COCO_MAX_DETS)


def test_update_from_slab_does_not_synchronise_and_compute_raises_on_status():
    """the launch is captured into a graph together with the evaluator's own device-side bookkeeping: a synchronisation or a copy to the host inside update_from_slab
    would make the capture fail; a stale row / a bad label surface in compute()"""
    case = E.random_case(13, n_img=4, n_det=30, n_gt=6, C=5)
    slab, targets = _slab_and_targets(case)
    ev = M.GpuDetectionEvaluator(5)
    ev.update_from_slab(slab, targets)            # allocates the accumulators outside the capture
    want = ev.compute()
    ev2 = M.GpuDetectionEvaluator(5)
    ev2.update_from_slab(slab, targets)
    ev2._n_gt.zero_(); ev2._batches.clear(); ev2._images = 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev2.update_from_slab(slab, targets)
    g.replay()
    assert ev2.compute() == want == _host_dict([case], 5, M.COCO_MAX_DETS)
    for bad, err in ((E.stale_case(), "stale shard"), (E.bad_label_case(), "outside")):
        ev = M.GpuDetectionEvaluator(bad["C"])
        ev.update_from_slab(*_slab_and_targets(bad))
        with pytest.raises(ValueError, match=err):
            ev.compute()
