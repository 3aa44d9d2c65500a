"""YOLOv5's validation matching on the MI355X: val_match_kernel through ops.val_match / ymi_val_match against the NumPy restatement of its contract in tests/_val_cases.py
-- match, tp and the confusion matrix equal, the IoU bit for bit -- and metrics.ConfusionMatrix / metrics.ValEvaluator against the host path fed the same inputs."""
import numpy as np
import pytest
import torch

import _val_cases as V
from yolort_amd import ops
from yolort_amd._lib import YmiError
from yolort_amd.utils import metrics as M

gpu = pytest.mark.gpu
DEV = "cuda"
IOUV = [float(t) for t in M.VAL_IOUV]
SIZES = (0, 1, 63, 64, 65, 1024)   # nothing, one, and both sides of a wave; the limit


def _dev(case):
    return [torch.from_numpy(case[k]).to(DEV) for k in ("boxes", "scores", "labels", "counts", "gt_boxes", "gt_labels", "gt_counts")]


def _check(case, conf, thrs, class_aware, all_fp=False, matrix=None, before=0):
    """one launch against the model; `matrix` / `before`: a device matrix that already holds `before`"""
    C = case["C"]
    matrix = torch.zeros(C + 1, C + 1, dtype=torch.int32, device=DEV) if matrix is None else matrix
    match, iou, tp, status = ops.val_match(*_dev(case), C, conf=conf, thrs=thrs, class_aware=class_aware, matrix=matrix, count_all_fp=all_fp)
    want = V.model(case, conf, thrs, class_aware, all_fp)
    np.testing.assert_array_equal(match.cpu().numpy(), want[0])
    np.testing.assert_array_equal(iou.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(tp.cpu().numpy(), want[2])
    np.testing.assert_array_equal(matrix.cpu().numpy(), want[3] + before)
    assert int(status[1]) == want[4]
    return want


@gpu
@pytest.mark.parametrize("G", SIZES)
@pytest.mark.parametrize("K", SIZES)
def test_sizes_against_the_model(K, G):
    case = V.random_case(1000 * K + G, K, G, C=80)
    want = _check(case, 0.25, [0.45], False)
    _check(case, float("-inf"), IOUV, True)
    if K >= 63 and G >= 63:
        assert (want[0] >= 0).any() and want[3][:80, 80].sum() > 0 and want[3][80, :80].sum() > 0   # matches, false positives and misses all occur


@gpu
@pytest.mark.parametrize("class_aware,all_fp", [(False, False), (False, True), (True, False)])
def test_crafted_images(class_aware, all_fp):
    case = V.make_case(list(V.CRAFTED.values()), 3)
    match, _, _, matrix, status = _check(case, 0.25, [0.5, 0.75], class_aware, all_fp)
    assert {name: match[i, : case["counts"][i]].tolist() for i, name in enumerate(V.CRAFTED)} == {
        "displaced": [0, -1], "iou on thr0": [0] if class_aware else [-1], "zero area": [-1, 1], "score at conf": [-1, 0, -1], "no match": [-1, -1],
        "ties": [0, -1, -1], "bad label": [-1, -1], "confusion": [-1] if class_aware else [0]}
    # [2, 3]: the zero-area detection, and the no-match image's only without the quirk; [2, 0]: the confusion
    assert status == 1 and matrix[2, 3] == 1 + int(all_fp) and matrix[2, 0] == (0 if class_aware else 1)


@gpu
@pytest.mark.parametrize("C", [1, 80, 200])   # 200: 161 KB of counters do not fit in LDS -- the additions go straight to global memory
def test_two_launches_accumulate_into_one_matrix(C):
    a, b = V.random_case(5, 65, 20, C), V.random_case(6, 40, 9, C, n_img=5)
    b["counts"][0], b["counts"][1] = 45, -1   # a count above K (image 0 is full: its 40 slots are valid) and a stale row
    matrix = torch.zeros(C + 1, C + 1, dtype=torch.int32, device=DEV)
    first = _check(a, 0.25, [0.45], False, matrix=matrix)
    second = _check(b, 0.25, [0.45], False, matrix=matrix, before=first[3])
    assert second[4] == 2 | 4 and (second[0][1] == -1).all()


REFUSALS = {"k": dict(K=1025), "g": dict(G=1025), "classes": dict(C=4097), "thresholds": dict(thrs=[0.5] * 11), "threshold range": dict(thrs=[1.5]), "cpu": dict(cpu=True)}


@gpu
@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(what):
    kw = dict(dict(K=4, G=4, C=4, thrs=[0.5], cpu=False), **REFUSALS[what])
    args = _dev(V.make_case([([], [], [], [], [])], kw["C"], kw["K"], kw["G"]))   # one empty image in a slab of K slots and G ground truths
    if kw["cpu"]:
        args[4] = args[4].cpu()
    with pytest.raises(YmiError, match=None if kw["cpu"] else "code -1"):
        ops.val_match(*args, kw["C"], conf=0.25, thrs=kw["thrs"], class_aware=False)


@gpu
def test_graph_capture_and_replays():
    args = _dev(V.random_case(8, 70, 12, C=5))
    matrix, status = torch.zeros(6, 6, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    kw = dict(conf=0.25, thrs=IOUV, class_aware=False, matrix=matrix, status=status)
    eager = ops.val_match(*args, 5, **kw)
    once = matrix.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.val_match(*args, 5, **kw)
    for r in range(3):
        [t.zero_() for t in out[:3]]
        g.replay()
        assert all(torch.equal(x, y) for x, y in zip(out[:3], eager[:3])) and torch.equal(matrix, once * (r + 2))   # the capture itself launches nothing


@gpu
def test_confusion_matrix_process_batch_and_slab():
    case = V.random_case(9, 30, 8, C=6, n_img=4)
    want = V.model(case, 0.25, [0.45], False)[3]
    cm, cs = M.ConfusionMatrix(6), M.ConfusionMatrix(6)
    b, s, l, c, gb, gl, gc = _dev(case)
    cs.update_from_slab((b, s, l, c), (gb, gl, gc))
    for i in range(4):   # the reference's layouts, an image at a time
        k, g = int(case["counts"][i]), int(case["gt_counts"][i])
        cm.process_batch(torch.cat([b[i, :k], s[i, :k, None], l[i, :k, None].float()], 1), torch.cat([gl[i, :g, None].float(), gb[i, :g]], 1))
    np.testing.assert_array_equal(cm.matrix, want)
    np.testing.assert_array_equal(cs.matrix, want)
    assert want.sum() > 0 and M.ConfusionMatrix(6).matrix.sum() == 0


def _host_summary(cases):
    """the host path: the model's true-positive rows of every live slot and the ground-truth classes through metrics.val_summary"""
    tp, conf, pcls, tcls = [], [], [], []
    for case in cases:
        live = np.arange(case["scores"].shape[1])[None, :] < case["counts"][:, None]
        tp.append(V.model(case, float("-inf"), IOUV, True)[2][live]); conf.append(case["scores"][live]); pcls.append(case["labels"][live])
        tcls.append(case["gt_labels"][np.arange(case["gt_labels"].shape[1])[None, :] < case["gt_counts"][:, None]])
    return M.val_summary(np.concatenate(tp), np.concatenate(conf), np.concatenate(pcls), np.concatenate(tcls))


@gpu
def test_val_evaluator_update_merge_compute():
    cases = [V.random_case(10, 120, 10, C=6, n_img=4), V.random_case(11, 64, 7, C=6)]
    want = _host_summary(cases)
    assert 0 < want["map"] < want["map50"] < 1 and len(want["ap_class"]) == 6
    ev, other = M.ValEvaluator(6), M.ValEvaluator(6)
    s0 = _dev(cases[0])
    ev.update_from_slab(tuple(s0[:4]), tuple(s0[4:]))
    c = cases[1]   # the list form
    preds = [{k: torch.from_numpy(c[k][i, :n]).to(DEV) for k in ("boxes", "scores", "labels")} for i, n in enumerate(c["counts"])]
    other.update(preds, [dict(boxes=c["gt_boxes"][i, :g], labels=c["gt_labels"][i, :g]) for i, g in enumerate(c["gt_counts"])])
    ev.merge(other)
    assert ev.compute() == want and M.ValEvaluator(6).compute()["map"] == 0.0


def test_ap_per_class_known_answer():
    """two of two found: recall (.5, 1), precision (1, 1) -> the 101-point interpolation is 1 up to its last point, where the sentinel (1, 0) takes over: the area is
    1 - 0.01 / 2 = 0.995, the reference's ceiling"""
    p, r, ap, f1, cls = M.ap_per_class(np.array([[1], [1]]), np.array([0.9, 0.8]), np.array([3, 3]), np.array([3, 3]))
    assert cls.tolist() == [3] and ap[0, 0] == pytest.approx(0.995, abs=1e-12) and p[0] == pytest.approx(1.0) and r[0] == pytest.approx(1.0)
