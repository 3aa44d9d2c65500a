"""Best-class post-process mode (include/yolort_amd.h YMI_POST_BEST_CLASS, `multi_label=False`: one label per anchor, ultralytics' non_max_suppression(...,
multi_label=False)) without a GPU: the Python surface and the plan key, the cases of tests/_best_cases.py checked against the oracle's decode for what they claim to reach,
decode_kernel and the fused head's epilogue on the CPU simulator (tests/hipsim: the unchanged simulator units run the new code, because the mode travels in CandSink through
make_sink) against the reference and against each other, and the sweep of the two properties of sigmoid_acc the fused head's class filter relies on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import _best_cases as B
import _head_cases as H
import _post_cases
from test_hipsim_kernels import Buf, _check, _clangxx, _conv_desc, sim  # noqa: F401  (sim: the module-scoped fixture that builds the simulator library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -3.0
# candidate capacity per image of the simulator runs.  The simulator library is ONE per process and remembers the largest dynamic LDS size any launch asked for
# (sim_max_lds), which tests of tests/test_hipsim_kernels.py assert on (<= 64 KiB after their own launches): with 4096 records per image the per-image sort stays at
# 32 KiB -- and no run here asks for the exact full pass, whose 16384-key sort takes 128 KiB -- so these tests leave that figure alone whatever the order of the modules.
SIM_CAP = 4096


# ---- host logic ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_constants_and_abi_version():
    from yolort_amd import _lib
    assert _lib.POST_BEST_CLASS == 2 == B.POST_BEST_CLASS and _lib.POST_EXACT_FULL == 1
    header = open(os.path.join(ROOT, "include", "yolort_amd.h")).read()
    assert "#define YMI_POST_BEST_CLASS 2" in header and "#define YMI_POST_EXACT_FULL 1" in header
    lib = _lib.load(require_gpu=False)
    assert lib.ymi_abi_version() == 6   # no layout or signature changed: a caller built against the previous header keeps working


def test_multi_label_kwarg_reaches_the_post_process():
    import yolort_amd.models as M
    from yolort_amd.models import yolo
    from yolort_amd.models.box_head import PostProcess
    assert PostProcess([8, 16, 32], 0.25, 0.45, 300).multi_label is True            # the default is the reference's multi-label contract
    assert PostProcess([8, 16, 32], 0.25, 0.45, 300, multi_label=False).multi_label is False
    assert PostProcess([8, 16, 32], 0.25, 0.45, 300, False).multi_label is False
    for make in (lambda **kw: yolo.yolov5_darknet_pan_n_r60(**kw), lambda **kw: M.YOLOv5(arch="yolov5_darknet_pan_n_r60", **kw).model, lambda **kw: M.yolov5n(**kw).model,
                 lambda **kw: yolo.YOLO(yolo.darknet_pan_backbone("darknet_n_r6_0", 0.33, 0.25, version="r6.0"), 80, **kw)):
        assert make().post_process.multi_label is True
        m = make(multi_label=False, score_thresh=0.3)
        assert m.post_process.multi_label is False and m.post_process.score_thresh == 0.3
    import inspect
    assert inspect.signature(yolo.YOLO.load_from_yolov5).parameters["multi_label"].default is True
    from yolort_amd import ops
    assert inspect.signature(ops.postprocess_logits).parameters["multi_label"].default is True


def test_the_plan_key_differs_between_the_modes():
    """flipping `post_process.multi_label` on a live model must not meet a plan recorded for the other mode: the value is part of the key, fused and unfused head alike"""
    from yolort_amd.models import yolo
    m = yolo.yolov5_darknet_pan_n_r60(score_thresh=0.25)
    assert m.fused()
    k_multi = m._post_key()
    m.post_process.multi_label = False
    k_best = m._post_key()
    assert k_multi != k_best and k_multi[:3] == k_best[:3] == (0.25, 0.45, 300)
    m.post_process.multi_label = True
    assert m._post_key() == k_multi
    m.fuse_head_decode = False
    assert m._post_key() == k_multi   # (the head form is a separate part of the key)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.EXISTING + B.NEW_CASES)
def test_cases_are_not_vacuous(name):
    print(B.assert_best_case_is_not_vacuous(name))


def test_reference_on_a_hand_made_prediction():
    """the restatement of general.py:572-583 itself: first maximal index, strict threshold, one record per anchor"""
    pred = torch.zeros(1, 4, 5 + 3)
    pred[0, :, :4] = torch.tensor([[10., 10., 4., 4.], [30., 10., 4., 4.], [50., 10., 4., 4.], [70., 10., 4., 4.]])
    pred[0, :, 4] = torch.tensor([0.5, 0.5, 1.0, 0.5])
    pred[0, :, 5:] = torch.tensor([[0.2, 0.8, 0.8], [1.0, 1.0, 0.0], [0.5, 0.1, 0.2], [0.2, 0.2, 0.2]])
    (r,) = B.best_postprocess(pred, 0.3, 1.0, 10)
    assert r["labels"].tolist() == [0, 0, 1] and r["scores"].tolist() == [0.5, 0.5, 0.4000000059604645]   # anchor 1 and 2 tie at 0.5: anchor order; anchor 3 fails
    (r,) = B.best_postprocess(pred, 0.5, 1.0, 10)
    assert len(r["scores"]) == 0                                                                            # conf == thr yields nothing


# ---- the simulator ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _post_desc(sim, n, nc, shapes, strides, anchors, thr, nms, k, cap, flags, logits=None):
    from yolort_amd._lib import PostDesc
    total_anchors = sum(3 * h * w for h, w in shapes)
    out = dict(boxes=torch.full((n, k, 4), FILL), scores=torch.full((n, k), FILL), labels=torch.full((n, k), int(FILL), dtype=torch.int64),
               count=torch.full((n,), int(FILL), dtype=torch.int32), status=torch.full((8,), int(FILL), dtype=torch.int32),
               ws=torch.full((int(sim.ymi_postprocess_ws_bytes(n, total_anchors, cap)),), 0x7f, dtype=torch.uint8))   # a dirty workspace
    d = PostDesc()
    for i, (h, w) in enumerate(shapes):
        d.lh[i], d.lw[i], d.stride[i] = h, w, float(strides[i])
        for j in range(6):
            d.anchors[i][j] = float(anchors[i][j])
        if logits is not None:
            d.logits[i], d.lcstride[i] = logits[i].data_ptr(), logits[i].shape[3]
    d.num_levels, d.n, d.num_classes = len(shapes), n, nc
    d.score_thresh, d.nms_thresh, d.detections_per_img = thr, nms, k
    d.out_boxes, d.out_scores, d.out_labels, d.out_count = out["boxes"].data_ptr(), out["scores"].data_ptr(), out["labels"].data_ptr(), out["count"].data_ptr()
    d.status, d.ws, d.ws_bytes, d.cand_cap, d.flags = out["status"].data_ptr(), out["ws"].data_ptr(), out["ws"].numel(), cap, flags
    return d, out


def _nhwc_logits(heads, nc):
    kk, out = nc + 5, []
    for ho in heads:
        n, _, h, w, _ = ho.shape
        t = torch.zeros(n, h, w, (3 * kk + 3) // 4 * 4, dtype=torch.float32)
        t[..., : 3 * kk] = ho.permute(0, 2, 3, 1, 4).reshape(n, h, w, 3 * kk)
        out.append(t)
    return out


def _sim_unfused(sim, heads, nc, strides, anchors, thr, nms, k, cap, flags):
    logits = _nhwc_logits(heads, nc)
    d, out = _post_desc(sim, heads[0].shape[0], nc, [(ho.shape[2], ho.shape[3]) for ho in heads], strides, anchors, thr, nms, k, cap, flags, logits)
    _check(sim, sim.ymi_postprocess(C.byref(d), None))
    return out


@pytest.mark.parametrize("nc", [1, 3, 80, 171])
def test_decode_kernel_best_class_vs_reference(sim, nc):
    """ymi_postprocess with YMI_POST_BEST_CLASS on random heads (three images; levels 10 x 12, 5 x 6, 3 x 3) against the restated reference: counts, labels, order exact,
    scores / boxes to the rounding of expf, status[4] = the number of passing anchors.  nc = 80: 255 channels, one float4 pass; nc = 171: 528 channels, three passes --
    a lane's running best crosses passes, and an anchor's classes spread over all of them.  nc = 1: bit-identical to the flag-less run."""
    from oracle import yolov5_oracle as O
    shapes, thr, k = [(10, 12), (5, 6), (3, 3)], 0.3, 300
    strides, anchors = O.anchors_for(3)
    heads = _post_cases.post_heads(nc, shapes)
    pred = O.decode(heads, strides, anchors)
    ref = B.best_postprocess(pred, thr, 0.45, k)
    conf = (pred[..., 5:] * pred[..., 4:5]).max(-1).values
    passing = int((conf > thr).sum())
    multi = int(((pred[..., 5:] * pred[..., 4:5]) > thr).sum())
    print(f"nc={nc}: passing anchors {passing}, multi-label candidates {multi}, detections {[len(r['scores']) for r in ref]}")
    assert passing > 30 and (nc == 1 or multi > passing)
    lds_before = sim.sim_max_lds()
    out = _sim_unfused(sim, heads, nc, strides, anchors, thr, 0.45, k, SIM_CAP * 3, B.POST_BEST_CLASS)
    assert sim.sim_max_lds() <= max(lds_before, 64 * 1024)   # (see SIM_CAP)
    st = out["status"].tolist()
    assert st[1] == 0 and st[4] == passing, st
    H.assert_equals_oracle(out, ref, FILL)
    if nc == 1:
        plain = _sim_unfused(sim, heads, nc, strides, anchors, thr, 0.45, k, SIM_CAP * 3, 0)
        for key in ("count", "labels", "scores", "boxes", "status"):
            assert torch.equal(plain[key], out[key]), key


@pytest.mark.parametrize("name", B.SIM_HEAD_CASES)
def test_fused_head_best_class_vs_reference_and_decode_kernel(sim, name):
    """conv_head_decode_group_kernel with YMI_POST_BEST_CLASS on the exact-logit cases that name a mistake (equal products from unequal logits, padding rows, box and
    objectness rows, equal logits across lane halves and sub-tiles; TNA = 1 at nc = 3 / 5, TNA = 3 at nc = 60) against the restated reference, and against ymi_postprocess
    (decode_kernel) on the same logits bit for bit.  Passes under both lane orders (HIPSIM_REVERSE=1)."""
    from yolort_amd._lib import ACT_NONE, ConvDesc, dtype_code
    print(B.assert_best_case_is_not_vacuous(name))
    case, want = B.best_case(name), B.best_reference(name)
    cpu, dtype, n, k, nc = torch.device("cpu"), case["dtype"], case["n"], case["k"], case["nc"]
    shapes, nl, cap, flags = case["shapes"], len(case["shapes"]), SIM_CAP * n, B.POST_BEST_CLASS
    head = H.make_head(case)
    xs = [Buf(n, h, w, c, dtype, fill=torch.from_numpy(x)) for x, c, (h, w) in zip(case["x"], case["chans"], shapes)]
    d, got = _post_desc(sim, n, nc, shapes, case["strides"], case["anchors"], case["thr"], case["nms"], k, cap, flags)
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
    conf = (case["pred"][..., 5:] * case["pred"][..., 4:5]).max(-1).values
    st = got["status"].tolist()
    assert st[1] == 0 and st[4] == int((conf > case["thr"]).sum()), st
    H.assert_equals_oracle(got, want, FILL)
    unfused = _sim_unfused(sim, case["logits"], nc, case["strides"], case["anchors"], case["thr"], case["nms"], k, cap, flags)
    for key in ("count", "labels", "scores", "boxes", "status"):
        assert torch.equal(unfused[key], got[key]), f"decode_kernel and the fused head differ in {key}"
    assert sim.sim_max_lds() <= max(lds_before, 64 * 1024)   # (see SIM_CAP)


# ---- the filter's assumptions ------------------------------------------------------------------------------------------------------------------------------------------
def test_sigmoid_properties_the_class_filter_relies_on(tmp_path):
    """best_class_cut (yolort_amd/csrc/post_common.hpp) evaluates exact scores only of the classes near the largest logit.  It does not assume sigmoid_acc monotone; it
    states two weaker properties, (A1) and (A2), and tests/best_class_sweep.cpp checks them for every pair of fp32 logits the filter can meet (every value with
    2^-12 <= |x| < 128 / 32, samples of every other binade) with the functions the kernels call.  The figures it finds are printed."""
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no host clang++ (ext_vector_type / _Float16 / __bf16 sources need clang)")
    exe = str(tmp_path / "best_class_sweep")
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unused-function", "-Wno-psabi", "-I", os.path.join(ROOT, "tests", "hipsim"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "yolort_amd", "csrc"), os.path.join(ROOT, "tests", "best_class_sweep.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
