"""Class filter of the post-process (include/yolort_amd.h YMI_POST_CLASS_FILTER, `classes=[...]`: ultralytics' non_max_suppression(..., classes=...),
yolort/v5/utils/general.py:585-587) without a GPU: the Python surface, validation and the plan key; the C entry points that are host code; from the oracle alone, that
the cases of tests/_classes_cases.py tell the stated semantics from its misreadings; and decode_kernel and the fused head's epilogue on the CPU simulator (tests/hipsim:
the unchanged simulator units run the new code -- the mask pointer travels in CandSink through make_sink, the mask itself is written into the host workspace at
ymi_post_class_mask_offset)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import _agnostic_cases as A
import _classes_cases as K
import _head_cases as H
import _post_cases
from test_best_class import SIM_CAP, _nhwc_logits, _post_desc
from test_hipsim_kernels import Buf, _check, _conv_desc, sim  # noqa: F401  (sim: the module-scoped fixture that builds the simulator library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -3.0
KEYS = ("count", "labels", "scores", "boxes", "status")


# ---- host logic ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_constants_and_abi_version():
    from yolort_amd import _lib
    assert _lib.POST_CLASS_FILTER == 8 == K.POST_CLASS_FILTER
    header = open(os.path.join(ROOT, "include", "yolort_amd.h")).read()
    assert "#define YMI_POST_CLASS_FILTER 8" in header and "is not provided" not in header and "general.py:585-587" in header
    lib = _lib.load(require_gpu=False)
    assert lib.ymi_abi_version() == 6   # no struct layout changed: the mask travels in the workspace
    for name in ("ymi_post_class_mask_offset", "ymi_post_set_classes", "ymi_plan_set_classes"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_mask_region_is_carved_last_and_aligned():
    from yolort_amd import _lib
    lib = _lib.load(require_gpu=False)
    for n, total_anchors, cap in ((3, 1890, 3 * 8192), (32, 25200, 1 << 19), (1, 12, 48), (64, 12, 64 * 48)):
        total, off = lib.ymi_postprocess_ws_bytes(n, total_anchors, cap), lib.ymi_post_class_mask_offset(n, total_anchors, cap)
        assert off > 0 and off % 256 == 0 and total - off >= 4 * K.MASK_WORDS == 512, (n, total_anchors, cap, total, off)
        assert total - off == 512   # the LAST region: everything in front of it is where it was
    assert lib.ymi_postprocess_ws_bytes(0, 25200, 10) == 0 and lib.ymi_post_class_mask_offset(0, 25200, 10) < 0


def test_set_classes_is_refused_without_the_flag_and_for_bad_indices():
    """validation is host code and comes first: nothing is launched for a refused call"""
    from yolort_amd import _lib
    lib = _lib.load(require_gpu=False)
    d = _lib.PostDesc()
    d.num_levels, d.n, d.num_classes, d.cand_cap = 1, 1, 80, 4096
    d.lh[0], d.lw[0] = 4, 4
    ws = (C.c_uint8 * int(lib.ymi_postprocess_ws_bytes(1, 48, 4096)))()
    d.ws, d.ws_bytes = C.addressof(ws), len(ws)
    one = (C.c_int32 * 2)(3, 79)
    d.flags = K.POST_BEST_CLASS | K.POST_AGNOSTIC
    assert lib.ymi_post_set_classes(C.byref(d), one, 2, None) == -1 and b"YMI_POST_CLASS_FILTER" in lib.ymi_last_error()
    d.flags |= K.POST_CLASS_FILTER
    for bad in (-1, 80):
        arr = (C.c_int32 * 2)(3, bad)
        assert lib.ymi_post_set_classes(C.byref(d), arr, 2, None) == -1 and b"class index" in lib.ymi_last_error()
    assert lib.ymi_post_set_classes(C.byref(d), None, 1, None) == -1
    assert lib.ymi_post_set_classes(None, one, 2, None) == -1
    assert lib.ymi_plan_set_classes(None, one, 2, None) == -1 and b"ymi_plan_set_classes" in lib.ymi_last_error()
    p = lib.ymi_plan_create()
    try:   # a plan without a filtered post-process
        assert lib.ymi_plan_set_classes(p, one, 2, None) == -1 and b"YMI_POST_CLASS_FILTER" in lib.ymi_last_error()
    finally:
        lib.ymi_plan_destroy(p)


def test_classes_kwarg_reaches_the_post_process():
    import yolort_amd.models as M
    from yolort_amd import ops
    from yolort_amd.models import yolo
    from yolort_amd.models.box_head import PostProcess
    pp = PostProcess([8, 16, 32], 0.25, 0.45, 300)
    assert pp.classes is None                                                     # the default: no filter
    pp.classes = [7, 0, 7, 2]
    assert pp.classes == (0, 2, 7)                                                # a set: order and duplicates are irrelevant
    pp.classes = []
    assert pp.classes == ()
    assert list(inspect.signature(PostProcess.__init__).parameters)[-1] == "agnostic"   # the constructor keeps the parameter list it had: `classes` is an attribute
    for make in (lambda **kw: yolo.yolov5_darknet_pan_n_r60(**kw), lambda **kw: M.YOLOv5(arch="yolov5_darknet_pan_n_r60", **kw).model, lambda **kw: M.yolov5n(**kw).model,
                 lambda **kw: yolo.YOLO(yolo.darknet_pan_backbone("darknet_n_r6_0", 0.33, 0.25, version="r6.0"), 80, **kw)):
        assert make().post_process.classes is None
        m = make(classes=range(3), score_thresh=0.3, multi_label=False)
        assert m.post_process.classes == (0, 1, 2) and m.post_process.score_thresh == 0.3 and m.post_process.multi_label is False
        with pytest.raises(ValueError):
            make(classes=[80])                                                        # num_classes itself
    assert inspect.signature(yolo.YOLO.load_from_yolov5).parameters["classes"].default is None
    assert inspect.signature(ops.postprocess_logits).parameters["classes"].default is None


def test_invalid_class_sets_raise_value_error():
    from yolort_amd.models import yolo
    from yolort_amd.models.box_head import PostProcess
    for bad in ([-1], [1.5], ["person"], [None], 3, "01"):
        with pytest.raises(ValueError):
            PostProcess([8, 16, 32], 0.25, 0.45, 300).classes = bad
        with pytest.raises(ValueError):
            yolo.yolov5_darknet_pan_n_r60(classes=bad)
    m = yolo.yolov5_darknet_pan_n_r60(num_classes=5)
    with pytest.raises(ValueError):
        m.post_process.classes = [-1]
    m.post_process.classes = [np.int64(4), torch.tensor(1)]     # integer-likes are indices
    assert m.post_process.classes == (1, 4) and m._post_key() is not None
    m.post_process.classes = [5]                                  # num_classes: the post-process does not know the class count, the model's next batch does
    with pytest.raises(ValueError):
        m._post_key()                                             # (what every submission evaluates first)
    own = PostProcess([8, 16, 32], 0.25, 0.45, 300)
    backbone = yolo.darknet_pan_backbone("darknet_n_r6_0", 0.33, 0.25, version="r6.0")
    with pytest.raises(ValueError):                               # an injected post-process is taken as it is: a set given next to it is refused, not dropped
        yolo.YOLO(backbone, 80, post_process=own, classes=[0])
    assert yolo.YOLO(backbone, 80, post_process=own).post_process is own


def test_the_plan_key_knows_whether_there_is_a_filter_but_not_the_set():
    """None <-> a set selects another plan (the flag is baked into the descriptor); a different SET must meet the same plan: the set is data in its workspace"""
    from yolort_amd.models import yolo
    m = yolo.yolov5_darknet_pan_n_r60(score_thresh=0.25)
    assert m.fused()
    k_none = m._post_key()
    m.post_process.classes = K.SET_A
    k_a = m._post_key()
    m.post_process.classes = K.SET_B
    k_b = m._post_key()
    m.post_process.classes = []
    k_empty = m._post_key()
    assert k_none != k_a and k_a == k_b == k_empty
    m.post_process.classes = None
    assert m._post_key() == k_none == (0.25, 0.45, 300, True, False)   # a model without a filter keeps the key it had
    m.post_process.classes = K.SET_A
    m.post_process.multi_label = False
    assert m._post_key() != k_a and m._post_key()[:3] == (0.25, 0.45, 300)


def test_reference_on_a_hand_made_prediction():
    """the restatement itself: the best class over ALL classes, the filter after the candidates and before the NMS"""
    pred = torch.zeros(1, 3, 5 + 3)
    pred[0, :, :4] = torch.tensor([[10., 10., 8., 8.], [11., 10., 8., 8.], [50., 10., 4., 4.]])
    pred[0, :, 4] = 1.0
    pred[0, :, 5:] = torch.tensor([[0.9, 0.6, 0.1], [0.2, 0.1, 0.8], [0.4, 0.7, 0.5]])
    kw = dict(thr=0.3, nms=0.45, k=10)
    (r,) = K.filtered_reference(pred, best=False, agnostic=False, classes=(1, 2), **kw)
    assert r["labels"].tolist() == [2, 1, 1, 2]                                    # 0.8, 0.7, 0.6, 0.5: class 0 is gone
    (r,) = K.filtered_reference(pred, best=True, agnostic=False, classes=(1, 2), **kw)
    assert r["labels"].tolist() == [2, 1]                                          # anchor 0's best class is 0: it yields NOTHING, although its class 1 passes
    (r,) = K.filtered_reference(pred, best=True, agnostic=False, classes=(1, 2), reading="allowed-argmax", **kw)
    assert r["labels"].tolist() == [2, 1, 1]                                       # the misreading keeps anchor 0 as class 1
    (r,) = K.filtered_reference(pred, best=True, agnostic=True, classes=(1, 2), **kw)
    assert r["labels"].tolist() == [2, 1]                                          # anchor 1 (0.8) survives: anchor 0 (0.9, class 0) is not there to suppress it
    (r,) = K.filtered_reference(pred, best=True, agnostic=True, classes=(1, 2), order="after", **kw)
    assert r["labels"].tolist() == [1]                                             # filtering after the NMS loses it
    (r,) = K.filtered_reference(pred, best=False, agnostic=False, classes=(), **kw)
    assert len(r["scores"]) == 0
    assert K.candidate_counts(pred, 0.3, False, (1, 2)) == [4] and K.candidate_counts(pred, 0.3, True, (1, 2)) == [2] and K.candidate_counts(pred, 0.3, True, None) == [3]
    assert K.mask_words((0, 31, 32, 4095))[[0, 1, 127]].tolist() == [0x80000001, 1, 0x80000000]


# ---- non-vacuity, from the oracle alone ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim_shapes", [False, True])
@pytest.mark.parametrize("nc", [2, 80])
def test_cases_tell_the_semantics_from_its_misreadings(nc, sim_shapes):
    """A.post_inputs(nc, "full"), GPU and simulator shapes, runs (0.3, 300), (0.05, 7), (0.05, 300), the sets the tests use:
      * k = 300: the filtered result differs from the unfiltered one in an image of every run, in every mode;
      * best-class: the stated semantics differ from "argmax over the allowed classes" in an image of every run;
      * agnostic: filter-before-NMS differs from filter-after-NMS in an image of every run with multi-label candidates, and of the (0.05, 300) run with best-class candidates;
      * class-aware multi-label: filter-before EQUALS filter-after in every image (per-class NMS commutes with the filter) -- what licenses the exact GPU-vs-GPU check."""
    sets = [K.set_a(nc)] + ([K.SET_B] if nc == 80 else [])
    for classes in sets:
        for thr, k in K.RUNS:
            for best in (False, True):
                for agnostic in (False, True):
                    got = A.cut(K.full_ref(nc, sim_shapes, thr, best, agnostic, classes), k)
                    plain = A.cut(A.post_full_ref(nc, "full", thr, best, agnostic, sim_shapes), k)
                    after = A.cut(K.full_ref(nc, sim_shapes, thr, best, agnostic, classes, "after"), k)
                    d_plain, d_after = A.differs(got, plain), A.differs(got, after)
                    print(f"nc={nc} sim={sim_shapes} |set|={len(classes)} thr={thr} k={k} best={best} agnostic={agnostic}: detections {[len(r['scores']) for r in got]} "
                          f"differ from unfiltered {d_plain}, from filter-after {d_after}")
                    assert all(set(r["labels"].tolist()) <= set(classes) for r in got)
                    if k == 300:
                        assert any(d_plain), "the filtered and the unfiltered result agree in every image"
                    # (best-class candidates are one per anchor and overlap less: at the higher threshold and in the seven-detection cut the two orders can agree in every
                    # image -- nc = 80, set A, (0.3, 300) does -- so with them the difference is asserted for the run that keeps the most boxes, (0.05, 300), in every set;
                    # the figures of the other runs are printed)
                    if agnostic and (not best or (thr, k) == (0.05, 300)):
                        assert any(d_after), "filter-before-NMS and filter-after-NMS agree in every image"
                    elif not best:
                        assert not any(d_after), "class-aware multi-label: the filter does not commute with the NMS"
                if best:   # once per run
                    stated = A.cut(K.full_ref(nc, sim_shapes, thr, True, False, classes), k)
                    misread = A.cut(K.full_ref(nc, sim_shapes, thr, True, False, classes, "before", "allowed-argmax"), k)
                    d = A.differs(stated, misread)
                    print(f"nc={nc} sim={sim_shapes} |set|={len(classes)} thr={thr} k={k}: best-class, stated vs argmax over the allowed classes differ {d}")
                    assert any(d), "the two readings of best-class mode agree in every image"


# ---- the simulator ---------------------------------------------------------------------------------------------------------------------------------------------------
def _write_mask(sim, out, n, total_anchors, cap, classes):
    """the consumer's way: the 128 words straight into the (host) workspace"""
    off = int(sim.ymi_post_class_mask_offset(n, total_anchors, cap))
    assert off > 0 and off + 512 <= out["ws"].numel()
    out["ws"][off: off + 512] = torch.from_numpy(K.mask_words(classes).view(np.uint8).copy())


def _sim_post(sim, heads, nc, strides, anchors, thr, k, cap, flags, classes):
    sim.ymi_post_class_mask_offset.argtypes, sim.ymi_post_class_mask_offset.restype = [C.c_int, C.c_int, C.c_int], C.c_int64
    logits = _nhwc_logits(heads, nc)
    shapes = [(ho.shape[2], ho.shape[3]) for ho in heads]
    n = heads[0].shape[0]
    d, out = _post_desc(sim, n, nc, shapes, strides, anchors, thr, 0.45, k, cap, flags | (K.POST_CLASS_FILTER if classes is not None else 0), logits)
    if classes is not None:
        _write_mask(sim, out, n, sum(3 * h * w for h, w in shapes), cap, classes)
    lds_before = sim.sim_max_lds()
    _check(sim, sim.ymi_postprocess(C.byref(d), None))
    assert sim.sim_max_lds() <= max(lds_before, 64 * 1024)   # (see test_best_class.SIM_CAP)
    return out


@pytest.mark.parametrize("best,agnostic", [(False, False), (True, False), (True, True)])
def test_decode_kernel_class_filter_vs_reference(sim, best, agnostic):
    """ymi_postprocess with YMI_POST_CLASS_FILTER at nc = 80, set A, (0.05, 300) on the simulator's levels, in multi-label mode, best-class mode and best-class + agnostic:
    counts, labels, order exact, scores / boxes to the rounding of expf; status[4] = the candidates AFTER the filter"""
    nc, thr, k, classes = 80, 0.05, 300, K.SET_A
    heads, strides, anchors, pred = A.post_inputs(nc, "full", True)
    ref = A.cut(K.full_ref(nc, True, thr, best, agnostic, classes), k)
    raw, unfiltered = sum(K.candidate_counts(pred, thr, best, classes)), sum(K.candidate_counts(pred, thr, best, None))
    print(f"best={best} agnostic={agnostic}: candidates {raw} of {unfiltered}, detections {[len(r['scores']) for r in ref]}")
    assert 0 < raw < unfiltered
    out = _sim_post(sim, heads, nc, strides, anchors, thr, k, SIM_CAP * 3, (K.POST_BEST_CLASS if best else 0) | (K.POST_AGNOSTIC if agnostic else 0), classes)
    st = out["status"].tolist()
    assert st[1] == 0 and st[4] == raw, st
    H.assert_equals_oracle(out, ref, FILL)


def test_decode_kernel_empty_set_gives_nothing(sim):
    heads, strides, anchors, pred = A.post_inputs(80, "full", True)
    out = _sim_post(sim, heads, 80, strides, anchors, 0.05, 300, SIM_CAP * 3, 0, ())
    st = out["status"].tolist()
    assert out["count"].tolist() == [0, 0, 0] and st[0] == 0 and st[1] == 0 and st[4] == 0, (out["count"], st)
    assert (out["scores"] == FILL).all() and (out["boxes"] == FILL).all()


def test_decode_kernel_one_class_is_bit_identical_to_no_filter(sim):
    heads, strides, anchors, pred = A.post_inputs(1, "full", True)
    plain = _sim_post(sim, heads, 1, strides, anchors, 0.3, 300, SIM_CAP * 3, 0, None)
    got = _sim_post(sim, heads, 1, strides, anchors, 0.3, 300, SIM_CAP * 3, 0, (0,))
    assert int(plain["count"].sum()) > 0
    for key in KEYS:
        assert torch.equal(plain[key], got[key]), key


def test_fused_head_class_filter_vs_reference(sim):
    """conv_head_decode_group_kernel on the lean twin of the dense case (9 classes, worklist and record buffer spill) with the mask {0, 3, 8}: the first class, the last, both
    lane halves (channels 5, 8 and 13) -- against the reference on the exact logits; status[4] = the filtered candidates"""
    from yolort_amd._lib import ACT_NONE, ConvDesc, dtype_code
    sim.ymi_post_class_mask_offset.argtypes, sim.ymi_post_class_mask_offset.restype = [C.c_int, C.c_int, C.c_int], C.c_int64
    case, classes = H.head_case("sim-dense"), (0, 3, 8)
    assert case["nc"] == 9 and {(c + 5) % 8 < 4 for c in classes} == {True, False}
    ref = K.filtered_reference(case["pred"], case["thr"], case["nms"], case["k"], False, False, classes)
    plain = H.head_reference("sim-dense")
    raw = sum(K.candidate_counts(case["pred"], case["thr"], False, classes))
    assert any(A.differs(ref, plain)) and 0 < raw < sum(case["candidates_per_image"])
    cpu, dtype, n, k, nc = torch.device("cpu"), case["dtype"], case["n"], case["k"], case["nc"]
    shapes, nl, cap = case["shapes"], len(case["shapes"]), SIM_CAP * n
    head = H.make_head(case)
    xs = [Buf(n, h, w, c, dtype, fill=torch.from_numpy(x)) for x, c, (h, w) in zip(case["x"], case["chans"], shapes)]
    d, got = _post_desc(sim, n, nc, shapes, case["strides"], case["anchors"], case["thr"], case["nms"], k, cap, K.POST_CLASS_FILTER)
    _write_mask(sim, got, n, sum(3 * h * w for h, w in shapes), cap, classes)
    arr, keep = (ConvDesc * nl)(), []
    for i, xb in enumerate(xs):
        pc = head.packed_anchor_major(i, dtype, cpu, case["chans"][i])
        keep.append(pc)
        cd = _conv_desc(xb, pc, xb, 0)
        cd.y, cd.y_cstride, cd.act, cd.out_dtype = None, 0, ACT_NONE, dtype_code(torch.float32)
        C.memmove(C.byref(arr, i * C.sizeof(ConvDesc)), C.byref(cd), C.sizeof(ConvDesc))
    lds_before = sim.sim_max_lds()
    _check(sim, sim.ymi_post_begin(C.byref(d), None))
    _check(sim, sim.sim_conv_head_decode_group(arr, nl, C.byref(d)))
    _check(sim, sim.ymi_post_finish(C.byref(d), None))
    assert sim.sim_max_lds() <= max(lds_before, 64 * 1024)
    st = got["status"].tolist()
    assert st[1] == 0 and st[4] == raw, (st, raw)
    H.assert_equals_oracle(got, ref, FILL)
