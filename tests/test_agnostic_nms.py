"""Class-agnostic NMS (include/yolort_amd.h YMI_POST_AGNOSTIC and ymi_nms; Python `agnostic=True`, ops.nms) without a GPU: the constants and the Python surface, the plan
key, the vacuity conditions of tests/_agnostic_cases.py from the oracle alone, and the workgroup-per-segment kernel (postprocess.hip nms_block_kernel) with its host routing
on the CPU simulator (tests/hipsim: postprocess.hip is a simulator unit, so the unchanged simulator library holds the new kernel and ymi_nms) against the oracle.
Every test of this file passes under both lane orders (HIPSIM_REVERSE=1)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import _agnostic_cases as A
import _head_cases as H
import _post_cases as P
from test_best_class import SIM_CAP, _nhwc_logits, _post_desc
from test_hipsim_kernels import _check, sim  # noqa: F401  (sim: the module-scoped fixture that builds the simulator library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -3.0


# ---- host logic ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_constants_and_abi_version():
    from yolort_amd import _lib
    assert _lib.POST_AGNOSTIC == 4 == A.POST_AGNOSTIC and _lib.POST_BEST_CLASS == 2 and _lib.POST_EXACT_FULL == 1
    header = open(os.path.join(ROOT, "include", "yolort_amd.h")).read()
    assert "#define YMI_POST_AGNOSTIC 4" in header and "int ymi_nms(const float* boxes, const float* scores, int n, float nms_thresh" in header
    assert "ymi_nms" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load(require_gpu=False)
    assert lib.ymi_abi_version() == 6   # a new flag value and a new function: a caller built against the previous header keeps working
    assert lib.ymi_nms.argtypes[2] is C.c_int and len(lib.ymi_nms.argtypes) == 9


def test_agnostic_kwarg_reaches_the_post_process():
    import yolort_amd.models as M
    from yolort_amd import ops
    from yolort_amd.models import yolo
    from yolort_amd.models.box_head import PostProcess
    assert PostProcess([8, 16, 32], 0.25, 0.45, 300).agnostic is False
    assert PostProcess([8, 16, 32], 0.25, 0.45, 300, agnostic=True).agnostic is True
    assert PostProcess([8, 16, 32], 0.25, 0.45, 300, False, True).agnostic is True           # the last positional parameter
    assert list(inspect.signature(PostProcess.__init__).parameters)[-1] == "agnostic"
    for make in (lambda **kw: yolo.yolov5_darknet_pan_n_r60(**kw), lambda **kw: M.YOLOv5(arch="yolov5_darknet_pan_n_r60", **kw).model, lambda **kw: M.yolov5n(**kw).model,
                 lambda **kw: yolo.YOLO(yolo.darknet_pan_backbone("darknet_n_r6_0", 0.33, 0.25, version="r6.0"), 80, **kw)):
        assert make().post_process.agnostic is False
        m = make(agnostic=True, multi_label=False, score_thresh=0.3)
        assert m.post_process.agnostic is True and m.post_process.multi_label is False and m.post_process.score_thresh == 0.3
    assert inspect.signature(yolo.YOLO.load_from_yolov5).parameters["agnostic"].default is False
    assert inspect.signature(ops.postprocess_logits).parameters["agnostic"].default is False
    assert list(inspect.signature(ops.nms).parameters) == ["boxes", "scores", "iou_threshold"]


def test_the_plan_key_differs_between_the_modes():
    """flipping `post_process.agnostic` on a live model must not meet a plan recorded for the other mode: the value is a NEW trailing element of the key, the first four
    stay what they were"""
    from yolort_amd.models import yolo
    m = yolo.yolov5_darknet_pan_n_r60(score_thresh=0.25)
    k_aware = m._post_key()
    assert k_aware == (0.25, 0.45, 300, True, False)
    m.post_process.agnostic = True
    k_agn = m._post_key()
    assert k_agn != k_aware and k_agn[:4] == k_aware[:4] and k_agn[4] is True
    m.post_process.multi_label = False
    assert m._post_key() == (0.25, 0.45, 300, False, True)
    m.post_process.agnostic, m.post_process.multi_label = False, True
    assert m._post_key() == k_aware


def test_ops_nms_refuses_cpu_tensors():
    from yolort_amd import ops
    from yolort_amd._lib import YmiError
    with pytest.raises(YmiError):
        ops.nms(torch.zeros(4, 4), torch.zeros(4), 0.5)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.NMS_CASES)
def test_nms_cases_differ_from_the_class_aware_result_exactly_where_listed(name):
    case, ref, aware = A.nms_case_and_refs(name)
    print(f"{name}: n={len(case['scores'])} agnostic keeps {len(ref)}, class-aware keeps {len(aware)}")
    assert (not np.array_equal(ref, aware)) == (name in A.NMS_DIFFER)


def test_length_and_spill_cases_are_not_vacuous():
    for n in A.LENGTHS:
        case, ref, aware = A.length_case(n)
        A.assert_length_case_is_not_vacuous(n, case, ref)
    case, ref = A.spill_case()
    print(f"spill: {len(case['scores'])} boxes, the oracle keeps {len(ref)} (LDS holds {A.NMSB_KCAP})")


@pytest.mark.parametrize("best", [False, True])
@pytest.mark.parametrize("nc", A.POST_NC)
def test_post_cases_are_not_vacuous(nc, best):
    for variant, thr, k in A.POST_RUNS:
        survivors, d = A.assert_post_case_is_not_vacuous(nc, variant, thr, k, best)
        print(f"nc={nc} best={best} {variant} thr={thr} k={k}: agnostic survivors {survivors}, images whose top-k differs from the class-aware one {d}")
    if nc == 80 and not best:
        pred = A.post_inputs(80, "full")[3]
        assert P.oracle_candidates_per_anchor(pred, 0.3).sum(1).tolist() == [6879, 6303, 7215]
        assert [len(r["scores"]) for r in A.post_full_ref(80, "full", 0.3, False)] == [295, 275, 294]   # below k = 300: the score prefix falls short


@pytest.mark.parametrize("best", [False, True])
def test_crowded_and_global_cases_are_not_vacuous(best):
    for aw, want in ((30.0, 855), (400.0, 8)):
        pred = A.crowded_inputs(aw)[3]
        assert len(A.post_reference(pred, 0.3, 0.45, 1 << 30, best)[0]["scores"]) == want
    for n, want in ((64, 63 if best else 64), (8, 8)):
        pred = A.global_inputs(n)[3]
        assert int(((pred[..., 5:] * pred[..., 4:5]) > A.GLOBAL["thr"]).sum((1, 2)).max()) <= 36 < A.GLOBAL["per_image_cap"]
        d = A.differs(A.post_reference(pred, 0.3, 0.45, 10, best), A.post_reference(pred, 0.3, 0.45, 10, best, agnostic=False))
        assert sum(d) == want, (n, best, sum(d))


# ---- the simulator -------------------------------------------------------------------------------------------------------------------------------------------------
def _sim_nms(sim, case):
    """ymi_nms on the simulator with a DIRTY workspace and pre-filled outputs -> (rc, keep, count)"""
    sim.ymi_nms.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    n = len(case["scores"])
    keep, count = np.full(max(n, 1), -7, np.int32), np.full(1, -7, np.int32)
    ws = np.full(int(sim.ymi_nms_ws_bytes(n)), 0x7f, np.uint8)
    rc = sim.ymi_nms(case["boxes"].ctypes.data, case["scores"].ctypes.data, n, C.c_float(case["thr"]), keep.ctypes.data, count.ctypes.data, ws.ctypes.data, ws.size, None)
    return rc, keep, count


def _assert_sim_nms(sim, case, ref):
    rc, keep, count = _sim_nms(sim, case)
    _check(sim, rc)
    c = int(count[0])
    np.testing.assert_array_equal(keep[:c].astype(np.int64), ref)
    assert (keep[c:] == -7).all(), "written past the count"


@pytest.mark.parametrize("name", A.SIM_NMS_CASES)
def test_nms_adversarial_vs_oracle(sim, name):
    """ymi_nms on signed zeros (a tie broken by index, four to a cell under two labels), IoU == threshold and 0/0 on the lattice, 257 equal scores, a 65 + 150 box input
    whose class-aware segments become one: kept indices equal the oracle's with every label equal, element for element"""
    case, ref, aware = A.nms_case_and_refs(name)
    assert (not np.array_equal(ref, aware)) == (name in A.NMS_DIFFER)
    _assert_sim_nms(sim, case, ref)


@pytest.mark.parametrize("n", A.LENGTHS)
def test_nms_segment_lengths_vs_oracle(sim, n):
    """the segment is the whole input: lengths around the 64-candidate step, the block size and twice the block size"""
    case, ref, aware = A.length_case(n)
    A.assert_length_case_is_not_vacuous(n, case, ref)
    _assert_sim_nms(sim, case, ref)


def test_nms_edge_calls(sim):
    """n == 0 leaves a count of 0 and touches nothing else; n = 2^20 is refused by name before anything is launched"""
    rc, keep, count = _sim_nms(sim, dict(boxes=np.zeros((0, 4), np.float32), scores=np.zeros(0, np.float32), thr=0.45))
    _check(sim, rc)
    assert int(count[0]) == 0 and (keep == -7).all()
    n = 1 << 20
    rc, keep, count = _sim_nms(sim, dict(boxes=np.zeros((n, 4), np.float32), scores=np.zeros(n, np.float32), thr=0.45))
    assert rc != 0 and "ymi_nms" in sim.sim_last_error().decode() and "out of range" in sim.sim_last_error().decode() and str(n - 1) in sim.sim_last_error().decode()
    assert int(count[0]) == -7 and (keep == -7).all()


def test_nms_spill_vs_oracle(sim):
    """7500 boxes of which 2500 are kept: 452 kept boxes live in the spill area (Workspace::kept_box) and are read back by every wave.  About 40 s on the simulator."""
    case, ref = A.spill_case()
    _assert_sim_nms(sim, case, ref)


def _sim_post(sim, heads, strides, anchors, nc, thr, k, cap, flags):
    """ymi_postprocess on the simulator under the host protocol of yolort_amd/ops.py (the mode flags stay set in every redo) -> (outputs of the last pass, status of every pass)"""
    logits = _nhwc_logits(heads, nc)
    n, passes = heads[0].shape[0], []
    while True:
        d, out = _post_desc(sim, n, nc, [(ho.shape[2], ho.shape[3]) for ho in heads], strides, anchors, thr, 0.45, k, cap, flags, logits)
        _check(sim, sim.ymi_postprocess(C.byref(d), None))
        st = out["status"].tolist()
        passes.append(st)
        assert len(passes) <= 4, passes
        if st[1] == 0:
            return out, passes
        assert st[1] & 1, "the simulator runs stay below the score-prefix selection (see SIM_CAP in tests/test_best_class.py)"
        need = max(st[0], st[3] * n)
        cap = max(int(need * 1.25) + 1024, 2 * cap)
        cap = n * (1 << ((cap + n - 1) // n - 1).bit_length())


@pytest.mark.parametrize("best", [False, True])
def test_postprocess_agnostic_vs_oracle(sim, best):
    """YMI_POST_AGNOSTIC through the per-image path (ranking sort with P = G, one segment per image, nms_block_kernel) at nc = 2 on three images, every run of
    A.POST_RUNS, multi-label and best-class candidates: counts, labels, order exact, scores / boxes to the rounding of expf, nothing written past the counts"""
    nc = 2
    lds_before = sim.sim_max_lds()
    for variant, thr, k in A.POST_RUNS:
        survivors, d = A.assert_post_case_is_not_vacuous(nc, variant, thr, k, best, sim=True)
        heads, strides, anchors, _ = A.post_inputs(nc, variant, sim=True)
        out, passes = _sim_post(sim, heads, strides, anchors, nc, thr, k, SIM_CAP * 3, A.POST_AGNOSTIC | (A.POST_BEST_CLASS if best else 0))
        print(f"best={best} {variant} thr={thr} k={k}: survivors {survivors} differ {d} passes {[p[:5] for p in passes]}")
        assert len(passes) == 1
        H.assert_equals_oracle(out, A.cut(A.post_full_ref(nc, variant, thr, best, True, sim=True), k), FILL)
    assert sim.sim_max_lds() <= max(lds_before, 64 * 1024)


def test_postprocess_agnostic_with_one_class_is_bit_identical_to_the_default(sim):
    heads, strides, anchors, _ = A.post_inputs(1, "full", sim=True)
    flagged, p1 = _sim_post(sim, heads, strides, anchors, 1, 0.3, 300, SIM_CAP * 3, A.POST_AGNOSTIC)
    plain, p0 = _sim_post(sim, heads, strides, anchors, 1, 0.3, 300, SIM_CAP * 3, 0)
    for key in ("count", "labels", "scores", "boxes", "status"):
        assert torch.equal(plain[key], flagged[key]), key
    assert int(plain["count"].sum()) > 30


@pytest.mark.parametrize("best", [False, True])
def test_postprocess_agnostic_global_sort_path_vs_oracle(sim, best):
    """cand_cap / n < 64: the global radix sort, make_label_records_kernel with label 0 and no label pass, segments = images; 8 images, every one of which differs
    from its class-aware result; no capacity growth (one pass, no overflow bit)"""
    n = 8
    heads, strides, anchors, pred = A.global_inputs(n)
    g = A.GLOBAL
    ref = A.post_reference(pred, g["thr"], 0.45, g["k"], best)
    out, passes = _sim_post(sim, heads, strides, anchors, g["nc"], g["thr"], g["k"], n * g["per_image_cap"], A.POST_AGNOSTIC | (A.POST_BEST_CLASS if best else 0))
    assert len(passes) == 1 and passes[0][1] == 0 and passes[0][2] == n, passes   # one segment per image
    H.assert_equals_oracle(out, ref, FILL)
