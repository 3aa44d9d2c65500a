"""On-device COCO matching (include/yolort_amd.h ymi_eval_match; Python ops.match_detections, metrics.GpuDetectionEvaluator) without a GPU: the header text, the exported
symbol and the Python surface, the host-side refusals, the vacuity conditions of tests/_eval_cases.py from the host oracle alone, the shared accumulation helper, and
eval_match_kernel on the CPU simulator (tests/hipsim: postprocess.hip is a simulator unit, so the unchanged simulator library holds the new kernel) against the oracle.
Every test of this file passes under both lane orders (HIPSIM_REVERSE=1)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import _eval_cases as E
from test_hipsim_kernels import _check, sim  # noqa: F401  (sim: the module-scoped fixture that builds the simulator library)
from yolort_amd.utils import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(case, out=None):
    """ymi_eval_desc over the case's numpy arrays (host pointers: the simulator, or a refusal that never reaches the device) -> (desc, outputs prefilled with sentinels)"""
    from yolort_amd._lib import EvalDesc
    N, K = case["scores"].shape
    G = case["gt_labels"].shape[1]
    R, T = len(case["rngs"]), len(case["thrs"])
    Ra = max(min(R, 4), 1)
    out = out or dict(tp=np.full((Ra, N, K), E.SENT16, np.uint16), ig=np.full((Ra, N, K), E.SENT16, np.uint16), rank=np.full((N, K), E.SENT_RANK, np.int32),
                      n_gt=np.full((Ra, case["C"]), E.SENT_NGT, np.int32), status=np.zeros(4, np.int32))
    d = EvalDesc()
    for k in ("boxes", "scores", "labels", "counts", "gt_boxes", "gt_labels", "gt_counts"):
        assert case[k].flags["C_CONTIGUOUS"]
        setattr(d, k, case[k].ctypes.data)
    for k in ("tp", "ig", "rank", "n_gt", "status"):
        setattr(d, k, out[k].ctypes.data)
    for i, t in enumerate(case["thrs"][:16]):
        d.thrs[i] = t
    for i, (lo, hi) in enumerate(case["rngs"][:4]):
        d.area_rng[i][0], d.area_rng[i][1] = lo, hi
    d.n, d.k, d.g, d.num_thrs, d.num_rngs, d.max_dets, d.num_classes = N, K, G, T, R, case["max_dets"] or 0, case["C"]
    return d, out


def _sim_run(sim, case, out=None):
    from yolort_amd._lib import EvalDesc
    sim.ymi_eval_match.argtypes, sim.ymi_eval_match.restype = [C.POINTER(EvalDesc), C.c_void_p], C.c_int
    d, out = _desc(case, out)
    _check(sim, sim.ymi_eval_match(C.byref(d), None))
    return out


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_and_abi_version():
    from yolort_amd import _lib
    header = open(os.path.join(ROOT, "include", "yolort_amd.h")).read()
    assert "typedef struct ymi_eval_desc {" in header and "int ymi_eval_match(const ymi_eval_desc* d, void* stream);" in header
    for word in ("#define YMI_EVAL_MAX_THRS 16", "#define YMI_EVAL_MAX_RNGS 4", "#define YMI_EVAL_MAX_PER_IMAGE 1024", "#define YMI_EVAL_STATUS_BAD_LABEL 1",
                 "#define YMI_EVAL_STATUS_STALE_ROW 2", "no crowd (iscrowd) ground truth", "#define YMI_ABI_VERSION 6"):
        assert word in header, word
    assert "ymi_eval_match" in _lib.EXPORTED_SYMBOLS
    assert (_lib.EVAL_MAX_THRS, _lib.EVAL_MAX_RNGS, _lib.EVAL_MAX_PER_IMAGE, _lib.EVAL_STATUS_BAD_LABEL, _lib.EVAL_STATUS_STALE_ROW) == (16, 4, 1024, 1, 2)
    lib = _lib.load(require_gpu=False)
    assert lib.ymi_abi_version() == 6   # a new struct and a new function: a caller built against the previous header keeps working
    assert lib.ymi_eval_match.argtypes[0]._type_ is _lib.EvalDesc and len(lib.ymi_eval_match.argtypes) == 2


def test_struct_layout_matches_the_header():
    import subprocess
    import tempfile
    from yolort_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "yolort_amd.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(ymi_eval_desc), offsetof(ymi_eval_desc, thrs), '
           'offsetof(ymi_eval_desc, area_rng), offsetof(ymi_eval_desc, n));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "s")], capture_output=True, text=True, check=True).stdout.split()]
    D = _lib.EvalDesc
    assert out == [C.sizeof(D), D.thrs.offset, D.area_rng.offset, D.n.offset]


def test_python_signatures():
    from yolort_amd import ops
    assert list(inspect.signature(ops.match_detections).parameters) == ["boxes", "scores", "labels", "counts", "gt_boxes", "gt_labels", "gt_counts", "num_classes",
                                                                         "iou_thrs", "area_rngs", "max_dets"]
    p = inspect.signature(ops.match_detections).parameters
    assert p["iou_thrs"].default is None and p["area_rngs"].default is None and p["max_dets"].default is None
    sig = inspect.signature(M.GpuDetectionEvaluator.__init__).parameters
    assert list(sig) == ["self", "num_classes", "max_dets"] and sig["num_classes"].default == 80 and sig["max_dets"].default == M.COCO_MAX_DETS
    for name in ("update", "update_from_slab", "merge", "compute"):
        assert list(inspect.signature(getattr(M.GpuDetectionEvaluator, name)).parameters) == list(inspect.signature(getattr(M.DetectionEvaluator, name)).parameters), name
    assert M.GpuDetectionEvaluator().compute() == M.DetectionEvaluator().compute() == {"AP": -1.0, "AP50": -1.0, "AP75": -1.0, "APs": -1.0, "APm": -1.0, "APl": -1.0}


def test_threshold_set_holds_the_host_evaluators_doubles():
    thrs, ap_idx, i50, i75 = M.eval_threshold_set()
    assert [thrs[i] for i in ap_idx] == [float(t) for t in M.COCO_IOU_THRS] and thrs[i50] == 0.5 and thrs[i75] == 0.75
    assert len(set(thrs)) == len(thrs) and 10 <= len(thrs) <= 12


def test_match_detections_refuses_cpu_tensors():
    from yolort_amd import ops
    from yolort_amd._lib import YmiError
    z = torch.zeros
    with pytest.raises(YmiError):
        ops.match_detections(z(1, 2, 4), z(1, 2), z(1, 2, dtype=torch.int64), z(1, dtype=torch.int32), z(1, 1, 4), z(1, 1, dtype=torch.int32), z(1, dtype=torch.int32), 3)
    ev = M.GpuDetectionEvaluator(num_classes=3)
    with pytest.raises(YmiError):
        ev.update_from_slab((z(1, 2, 4), z(1, 2), z(1, 2, dtype=torch.int64), z(1, dtype=torch.int32)), [{"boxes": z(0, 4), "labels": z(0, dtype=torch.int64)}])
    with pytest.raises(ValueError):
        ev.update_from_slab((z(2, 2, 4), z(2, 2), z(2, 2, dtype=torch.int64), z(2, dtype=torch.int32)), [{"boxes": z(0, 4), "labels": z(0, dtype=torch.int64)}])


REFUSALS = [("k", dict(K=1025), "k=1025"), ("g", dict(G=1025), "g=1025"), ("thresholds", dict(thrs=[0.5] * 17), "17 thresholds"),
            ("ranges", dict(rngs=[E.INF_RNG] * 5), "5 area ranges"), ("zero threshold", dict(thrs=[0.5, 0.0]), "outside (0, 1]")]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_carry_einval_before_anything_is_launched(what, kw, msg):
    """the product library without a GPU: the arguments are validated on the host, before the device is touched"""
    from yolort_amd import _lib
    lib = _lib.load(require_gpu=False)
    base = dict(K=None, G=None, thrs=None, rngs=E.COCO_RNGS)
    base.update(kw)
    case = E.make_case([(np.zeros((1, 4)), np.ones(1, np.float32), np.zeros(1, np.int64))], [(np.zeros((1, 4)), np.zeros(1, np.int32))], C=2, **base)
    d, out = _desc(case)
    assert lib.ymi_eval_match(C.byref(d), None) == -1 and msg in lib.ymi_last_error().decode(), lib.ymi_last_error().decode()
    assert (out["tp"] == E.SENT16).all() and (out["rank"] == E.SENT_RANK).all() and (out["n_gt"] == E.SENT_NGT).all()


# ---- the shared accumulation ---------------------------------------------------------------------------------------------------------------------------------------
def test_shared_accumulation_reproduces_coco_ap():
    """coco_ap goes through _ap_per_threshold; rebuilt from the flag oracle and the same helper it gives the same double -- the path GpuDetectionEvaluator.compute() takes"""
    case = E.random_case(7, n_img=4, n_det=40, n_gt=6, C=5, max_dets=10)
    preds, targets = E.to_lists(case)
    for t in targets:
        t["scores"] = np.ones(len(t["labels"]), np.float32)
    thrs = np.asarray(M.COCO_IOU_THRS)
    for rng in (None, M.COCO_AREA_RNG["small"], M.COCO_AREA_RNG["medium"]):
        want = M.coco_ap(targets, preds, 5, max_dets=10, area_rng=rng)
        aps = []
        for c in range(5):
            sc, tp, ig, n_gt = [], [], [], 0
            for p, t in zip(preds, targets):
                m = p["labels"] == c
                order, tpf, igf, ng, _ = E.match_one(t["boxes"][t["labels"] == c], p["boxes"][m], p["scores"][m], thrs, 10, E.INF_RNG if rng is None else rng)
                sc.append(p["scores"][m][order].astype(np.float64)); tp.append(tpf); ig.append(igf); n_gt += ng
            if n_gt == 0:
                continue
            aps.append(float(np.mean(M._ap_per_threshold(np.concatenate(sc), np.concatenate(tp), np.concatenate(ig), n_gt))) if len(np.concatenate(sc)) else 0.0)
        assert want is not None and want == float(np.mean(aps)), (rng, want, float(np.mean(aps)))


# ---- the cases are not vacuous (host oracle alone) -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ng", E.LANE_WRAP)
def test_lane_wrap_cases_are_not_vacuous(ng):
    exp = E.expected(E.lane_wrap_case(ng))
    gm = exp["gm"][0, 0, :, 0]                                   # range all, threshold 0.5
    assert sorted(gm[:ng].tolist()) == list(range(ng))           # every ground truth is taken, the last one included (position ng - 1: beyond lane 63 from 65 on)
    assert gm[ng] == -1 and not exp["tp"][0, 0, ng] & 1          # the low-scored copy of the last ground truth finds it used at 0.5 ...
    assert exp["gm"][0, 0, ng, -1] == ng - 1 and exp["gm"][0, 0, ng - 1, -1] == -1   # ... and free at 0.95, where the shifted box (IoU 81 / 119) no longer matches
    assert exp["rank"][0, ng - 1] == 0 and exp["n_gt"][0, 0] == ng + E.SENT_NGT


def test_detection_count_cases_are_not_vacuous():
    per = {(0, 1): 1, (0, 2): 99, (0, 3): 100, (1, 4): 101, (1, 5): 150}
    for max_dets, kept in ((100, lambda n: min(n, 100)), (2, lambda n: min(n, 2)), (None, lambda n: n)):
        case = E.det_counts_case(max_dets)
        assert case["scores"].shape == (2, 300) and case["counts"].tolist() == [200, 251]
        exp = E.expected(case)
        for (i, c), n in per.items():
            m = case["labels"][i, : case["counts"][i]] == c
            assert int(m.sum()) == n and int((exp["rank"][i, : case["counts"][i]][m] >= 0).sum()) == kept(n)
        assert (case["labels"][:, :200] != 0).all() and exp["n_gt"][0, 0] == 6 + E.SENT_NGT        # class 0: ground truth and no detection
    cut = E.expected(E.det_counts_case(100))
    case = E.det_counts_case(100)
    m = np.nonzero(case["labels"][1, :251] == 4)[0]
    assert (cut["rank"][1, m] == -1).sum() == 1 and case["scores"][1, m][cut["rank"][1, m] == -1] == case["scores"][1, m].min()   # the 101st: the lowest score
    assert not (np.diff(case["scores"][1, :251]) <= 0).all()                                                                      # the slab is not sorted


def test_score_order_case_is_not_vacuous():
    case = E.score_order_case()
    exp = E.expected(case)
    assert np.argsort(exp["rank"][0]).tolist() == E.SCORE_ORDER and np.signbit(case["scores"][0, [1, 4]]).all() and not np.signbit(case["scores"][0, 0])
    assert (exp["tp"][0, 0] != 0).tolist() == [False, False, True, False, False]


def test_iou_boundary_case_is_not_vacuous():
    case = E.iou_boundary_case()
    exp = E.expected(case)
    thrs = np.asarray(case["thrs"])
    iou = M._iou_matrix(case["boxes"][0, :2], case["gt_boxes"][0, :1])[:, 0]
    assert iou.dtype == np.float32 and iou.tolist() == [0.5, 0.75] and 0.5 in case["thrs"] and 0.75 in case["thrs"]
    for slot, v in ((0, 0.5), (1, 0.75)):
        bits = [(int(exp["tp"][0, 0, slot]) >> t) & 1 for t in range(len(thrs))]
        assert bits == [int(t <= v) for t in thrs] and 0 < sum(bits) < len(thrs)    # at that threshold and below, not at the next


def test_iou_tie_and_greedy_cases_are_not_vacuous():
    case = E.iou_tie_case()
    exp = E.expected(case)
    iou = M._iou_matrix(case["boxes"][0, :1], case["gt_boxes"][0, :2])[0]
    assert iou[0] == iou[1] and exp["gm"][0, 0, 0, 0] == 1 and exp["gm"][0, 0, 1, 0] == 0      # two equal maximal IoUs: the oracle takes the later one
    case = E.greedy_case()
    exp = E.expected(case)
    iou = M._iou_matrix(case["boxes"][0, :2], case["gt_boxes"][0, :1])[:, 0]
    tp0, tp1 = int(exp["tp"][0, 0, 0]), int(exp["tp"][0, 0, 1])
    assert iou[1] > iou[0] >= 0.5 and tp0 == 0b111 and not tp1 & tp0 and exp["ig"][0, 0, 1] == 0    # 0.5 .. 0.6: the better box finds the ground truth used
    assert tp1 == 0b11111000      # it gets it from 0.65 on, where the first no longer matches; not at 0.9: float32(0.9) < 0.8999999999999999


def test_area_case_is_not_vacuous():
    case = E.area_case()
    exp = E.expected(case)
    ALL, S, Md, L = 0, 1, 2, 3
    assert exp["gm"][ALL, 0, 0, 0] == 1 and exp["gm"][S, 0, 0, 0] == 0                         # all: the better (medium) ground truth; small: the worse, non-ignored one
    assert exp["tp"][S, 0, 0] & 1 and exp["n_gt"][S, 0] - E.SENT_NGT == 1 and exp["n_gt"][ALL, 0] - E.SENT_NGT == 2   # ignored in small, not in all
    assert exp["ig"][S, 0, 1] != 0 and exp["ig"][L, 0, 1] != 0 and exp["ig"][Md, 0, 1] == 0 and exp["ig"][ALL, 0, 1] == 0 and (exp["tp"][:, 0, 1] == 0).all()
    area = M._area(case["gt_boxes"][0, 2:4])
    assert area.tolist() == [1024.0, 9216.0]
    assert (exp["n_gt"][:, 1] - E.SENT_NGT).tolist() == [2, 1, 2, 1]                           # 1024 counts in small AND medium, 9216 in medium AND large
    assert exp["ig"][S, 0, 2] & 1 and exp["tp"][S, 0, 2] == 0 and exp["tp"][Md, 0, 2] & 1      # matched to an ignored ground truth


def test_degenerate_case_is_not_vacuous():
    case = E.degenerate_case()
    exp = E.expected(case)
    iou = M._iou_matrix(case["boxes"][0, :4], case["gt_boxes"][0, :3])
    assert iou[0, 0] == 0 and not (iou[:3] > 0).any() and iou[3, 2] >= 0.5 and M._area(case["gt_boxes"][0, 1:2])[0] < 0
    assert (exp["tp"][:, 0, :3] == 0).all() and exp["tp"][0, 0, 3] & 1
    assert (exp["n_gt"][:, 0] - E.SENT_NGT).tolist() == [3, 2, 0, 0]                           # the inverted box counts only where nothing is ignored


def test_nan_score_case_is_not_vacuous():
    case = E.nan_score_case()
    exp = E.expected(case)
    assert np.isnan(case["scores"][0, [17, 19]]).all() and case["counts"][0] == 20 and exp["status"] == 0
    assert exp["rank"][0, 16:20].tolist() == E.NAN_RANKS                                       # NaN last, in slab order among themselves
    assert exp["tp"][0, 0, 16] == (1 << len(case["thrs"])) - 1 and (exp["tp"][:, 0, 17:20] == 0).all()   # the 0.9 box takes the ground truth at every threshold
    assert (exp["tp"][0, 0, :16] & 1).all()


def test_ragged_and_status_cases_are_not_vacuous():
    case = E.random_case(9, n_img=33, n_det=12, n_gt=5, C=4, ragged=True)
    exp = E.expected(case)
    assert (case["counts"] == 0).any() and (case["gt_counts"] == 0).any() and len(set(case["counts"].tolist())) > 5
    assert np.isnan(case["boxes"][0, case["counts"][0]:]).all() and (case["labels"][0, case["counts"][0]:] == E.POISON_LABEL).all()
    assert exp["status"] == 0 and (exp["tp"][0] != 0).sum() > 20 and ((exp["ig"][1] != 0) & (exp["ig"][1] != E.SENT16)).sum() > 20
    live = exp["rank"] >= 0
    no_gt = (case["gt_counts"] == 0) & (case["counts"] > 0)                                   # images without ground truth that still hold detections: all unmatched
    assert no_gt.sum() >= 2 and live[no_gt].any() and (exp["tp"][:, no_gt][:, live[no_gt]] == 0).all()
    orphans = [(i, c) for i in range(33) for c in range(4) if case["gt_counts"][i] > 0 and (case["labels"][i, : case["counts"][i]] == c).any()
               and not (case["gt_labels"][i, : case["gt_counts"][i]] == c).any()]                 # a class with detections and no ground truth beside classes that have some
    assert len(orphans) >= 3 and all((exp["tp"][:, i][:, (case["labels"][i] == c) & live[i]] == 0).all() for i, c in orphans)
    one = E.random_case(8, n_img=1, n_det=40, n_gt=6, C=4)                                      # N = 1
    assert one["scores"].shape[0] == 1 and (E.expected(one)["tp"][0, 0, :40] != 0).sum() >= 4
    assert E.expected(E.bad_label_case())["status"] == 1 and E.expected(E.stale_case())["status"] == 2
    assert (E.expected(E.stale_case())["rank"][1] == E.SENT_RANK).all()


# ---- the simulator -------------------------------------------------------------------------------------------------------------------------------------------------
SIM_CASES = {
    "lane wrap 65": lambda: E.lane_wrap_case(65),
    "lane wrap 130": lambda: E.lane_wrap_case(130),
    "score order": E.score_order_case,
    "iou boundaries": E.iou_boundary_case,
    "iou tie": E.iou_tie_case,
    "greedy": E.greedy_case,
    "area ranges": E.area_case,
    "degenerate": E.degenerate_case,
    "max_dets 2": lambda: E.random_case(5, n_img=2, n_det=24, n_gt=4, C=3, max_dets=2),
    "ragged": lambda: E.random_case(9, n_img=5, n_det=12, n_gt=5, C=4, ragged=True, max_dets=None),
    "nan score": E.nan_score_case,
    "bad label": E.bad_label_case,
    "stale row": E.stale_case,
}


@pytest.mark.parametrize("name", list(SIM_CASES))
def test_eval_match_kernel_vs_oracle(sim, name):
    """ymi_eval_match on the simulator: every flag, rank, ground-truth count and status bit equals the host oracle's, and nothing but the defined slots is written"""
    case = SIM_CASES[name]()
    E.assert_outputs(case, _sim_run(sim, case))


def test_eval_match_accumulates_over_launches(sim):
    """n_gt is ADDED to and status ORed into: two launches on the halves equal one launch on the whole"""
    case = E.random_case(6, n_img=4, n_det=10, n_gt=4, C=3)
    a, b = E.split_case(case, 1)
    whole = _sim_run(sim, case)
    oa = _sim_run(sim, a)
    ob = _sim_run(sim, b, out=dict(tp=np.full_like(whole["tp"][:, 1:], E.SENT16), ig=np.full_like(whole["ig"][:, 1:], E.SENT16),
                                   rank=np.full_like(whole["rank"][1:], E.SENT_RANK), n_gt=oa["n_gt"], status=oa["status"]))
    np.testing.assert_array_equal(ob["n_gt"], whole["n_gt"])
    np.testing.assert_array_equal(np.concatenate([oa["tp"], ob["tp"]], 1), whole["tp"])
    np.testing.assert_array_equal(np.concatenate([oa["rank"], ob["rank"]]), whole["rank"])


def test_eval_match_edge_calls(sim):
    """n == 0 launches nothing; an image without a detection (one empty slot) still counts its ground truth"""
    from yolort_amd._lib import EvalDesc
    sim.ymi_eval_match.argtypes, sim.ymi_eval_match.restype = [C.POINTER(EvalDesc), C.c_void_p], C.c_int
    d = EvalDesc()
    d.num_thrs, d.num_rngs, d.num_classes = 1, 1, 1
    d.thrs[0] = 0.5
    _check(sim, sim.ymi_eval_match(C.byref(d), None))
    case = E.make_case([(np.zeros((0, 4)), np.zeros(0, np.float32), np.zeros(0, np.int64))], [(np.array([[0, 0, 4, 4]]), np.zeros(1, np.int32))], C=1)
    E.assert_outputs(case, _sim_run(sim, case))
