"""Augmented inference (test-time augmentation; include/yolort_amd.h ymi_scale_view / ymi_post_decode_view, Python `augment=True`) on the GPU: the cases of
tests/test_tta.py on the real kernels (same inputs, same expectations, integer outputs equal to the simulator's), the composition of the engine bit for bit, the whole
pipeline against the restated reference in fp32 mode, and the protocols (capacity growth, graphs off, a live toggle, an exported plan).  Yardsticks: tests/_tta_cases.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _tta_cases as T
import test_tta as CPU
from test_hipsim_kernels import sim  # noqa: F401
from test_merge_nms_gpu import _pack, _same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH, SEED, CANVAS, NMS = "yolov5_darknet_pan_n_r60", 7, T.CANVAS, 0.45


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from yolort_amd import _lib
    return _lib.load(require_gpu=True)


# ---- 7. items 2-5 on the device ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "mirror"])
@pytest.mark.parametrize("case", T.SCALE_CASES, ids=lambda c: f"{c[0]}x{c[1]}@{c[2]}")
def test_scale_kernel(dev, lib, case, flip, dt):
    h, w, ratio = case
    x = T.canvas(2, h, w, dt)
    got, ch3, guards = T.run_scale(lib, x, ratio, flip, dt, device=dev)
    T.check_scale(got, ch3, guards, x, ratio, flip, dt)


def test_ops_scale_image(dev):
    from yolort_amd import ops
    x = T.canvas(2, 128, 160, "f16").to(dev).half()
    for ratio, flip in ((0.83, True), (0.67, False), (1.0, True)):
        y = ops.scale_image(x, ratio, flip)
        ref = T.scale_img_ref(x.float().cpu(), ratio, flip) if ratio != 1.0 else x.float().cpu().flip(3)
        assert y.dtype == x.dtype and tuple(y.shape) == tuple(ref.shape)
        assert float((y.float().cpu() - ref).abs().max()) <= T.scale_tolerance("f16")
    with pytest.raises(ValueError):
        ops.scale_image(x, 1.5)


@pytest.mark.parametrize("nc", [1, 80])
@pytest.mark.parametrize("mode", ["multi", "best", "filter"])
def test_view_decode_equals_the_transformed_scale1_decode(dev, lib, nc, mode):
    CPU._view_decode_case(lib, nc, mode, dev)


@pytest.mark.parametrize("mode", list(CPU.ONE_BODY_MODES))
@pytest.mark.parametrize("nc,thr", CPU.ONE_BODY_PARAMS)
def test_scale1_view_decode_equals_the_plain_decode_bit_for_bit(dev, lib, nc, thr, mode):
    CPU._one_body_case(lib, nc, thr, mode, dev)


@pytest.mark.parametrize("flags,classes", [(0, None), (T.POST_BEST_CLASS, None), (T.POST_CLASS_FILTER, (1,))], ids=["multi", "best", "filter"])
def test_three_views_anchor_bases_and_tie_order(dev, lib, sim, flags, classes):
    """... and the integer outputs (counts, labels, status words) equal the simulator's run of the same inputs; so do scores and boxes of these exact-palette inputs"""
    out = CPU._union_case(lib, 2, flags, classes, dev)
    ref = CPU._union_case(sim, 2, flags, classes, "cpu")
    for key in ("count", "labels", "scores", "boxes"):
        assert torch.equal(out[key], ref[key]), key
    assert torch.equal(out["status"][:5], ref["status"][:5])


def test_tails_and_cross_view_ties(dev, lib):
    CPU._tie_and_tail_case(lib, dev, CPU.STRIDES3, CPU.ANCH3, T.CANVAS)
    CPU._tie_and_tail_case(lib, dev, CPU.STRIDES4, CPU.ANCH4, (128, 192))


@pytest.mark.parametrize("run", T.WHOLE_RUNS, ids=lambda r: f"nc{r[0]}-{'best' if r[4] else 'multi'}-{'agnostic' if r[5] else 'aware'}-{'filter' if r[6] else 'all'}-{'merge' if r[7] else 'plain'}")
def test_whole_post_process_of_three_views_vs_the_oracle(dev, lib, sim, run):
    out = CPU._whole_case(lib, run, dev)
    ref = CPU._whole_case(sim, run, "cpu")
    assert torch.equal(out["count"], ref["count"]) and torch.equal(out["labels"], ref["labels"]) and torch.equal(out["status"][:5], ref["status"][:5])   # integer outputs: exact


def test_ops_postprocess_logits_tta(dev, lib):
    """the public unit equals the driver's run of the same heads bit for bit (one case with a filter, agnostic and best-class mode together)"""
    from yolort_amd import ops
    nc, thr, k = 80, 0.3, 300
    view_heads, strides, anchors = T.whole_case(nc)
    classes = (0, 3, 17, 41, 79)
    dets = ops.postprocess_logits_tta([[h.to(dev) for h in hv] for hv in view_heads], T.SCALES, T.FLIPS, T.CANVAS, strides, anchors, nc, thr, NMS, k,
                                      multi_label=False, agnostic=True, classes=classes)
    views, _ = T.tta_views(view_heads, T.CANVAS[1])
    out = T.run_views(lib, views, 2, nc, strides, anchors, thr, NMS, k, 2 * 4096, T.run_flags(True, True, classes, False), classes, dev)
    assert sum(len(d["scores"]) for d in dets) > 10
    for i, d in enumerate(dets):
        b, s, lab = T.rows(out, i)
        assert np.array_equal(d["boxes"].cpu().numpy(), b) and np.array_equal(d["scores"].cpu().numpy(), s) and np.array_equal(d["labels"].cpu().numpy(), lab)


# ---- 8. composition, bit for bit ---------------------------------------------------------------------------------------------------------------------------------
def _core(dev, dtype, thr, **kw):
    """yolov5n with the conditioned recipe of workloads/; fp32 parameters with set_compute_dtype(fp32) = the fp32 mode"""
    from workloads.synth import conditioned_weights
    from yolort_amd.models import YOLOv5
    m = YOLOv5(arch=ARCH, size=CANVAS, score_thresh=thr, nms_thresh=NMS, **kw)
    m.load_state_dict(conditioned_weights(m.state_dict(), ARCH, SEED))
    m = m.to(dev).eval()
    if dtype == torch.float32:
        m.set_compute_dtype(torch.float32)
    else:
        m = m.to(dtype)
    return m


def _batch(dev, dtype, n=3):
    from workloads.synth import synth_images
    return synth_images(n, *CANVAS, seed=9).to(dev).to(dtype)


def _logits_of(core, x):
    """the stored fp32 logits the UNAUGMENTED model (stored-logits path) produces for the batch x, in the reference layout [(n, 3, h, w, K)]"""
    assert core.augment is False and core.fuse_head_decode is False
    core(x)
    torch.cuda.synchronize()
    e = next(iter(core._entries.values()))
    assert e.logits is not None and (e.x.h, e.x.w) == tuple(x.shape[2:])
    k = core.num_classes + 5
    return [v.as_tensor().clone().reshape(v.n, v.h, v.w, 3, k).permute(0, 3, 1, 2, 4).contiguous() for v in e.logits]


THRESHOLDS = (0.2, 0.15, 0.1, 0.08)   # (the conditioned recipe places its scores just under 0.26: the CPU reference of this batch has 234 / 606 candidates at 0.1, 60 000 at 0.05)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32-mode"])
def test_augment_equals_its_composition_bit_for_bit(dev, dtype):
    """augment=True on a (3, 3, 128, 160) batch == ops.postprocess_logits_tta of the logits that the unaugmented model (stored-logits path) produces for ops.scale_image of
    the same canvas at each view's size: same kernels on the same shapes, no tolerance.  Not vacuous: a kept detection's box is none of view 0's candidate boxes (its
    record comes from view 1 or 2), and the result differs from augment=False."""
    from yolort_amd import ops
    x = _batch(dev, dtype)
    for thr in THRESHOLDS:
        aug = _core(dev, dtype, thr, augment=True).model
        dets = aug(x)
        if all(len(d["scores"]) >= 3 for d in dets):
            break
    else:
        pytest.fail("no threshold of the list gives every image three detections")
    print("score_thresh", thr, "detections", [len(d["scores"]) for d in dets])
    plain = _core(dev, dtype, thr).model
    plain.fuse_head_decode = False
    strides = [float(s) for s in plain.anchor_generator.strides]
    anchors = plain.anchor_generator.anchor_grids
    view_outputs = [_logits_of(plain, x if r == 1.0 else ops.scale_image(x, r, f, gs=32)) for r, f in zip(T.SCALES, T.FLIPS)]
    assert [tuple(h.shape[2:4]) for h in view_outputs[2]] == [(12, 16), (6, 8), (3, 4)]
    want = ops.postprocess_logits_tta(view_outputs, T.SCALES, T.FLIPS, CANVAS, strides, anchors, plain.num_classes, thr, NMS, 300)
    assert _same(dets, want), [(len(a["scores"]), len(b["scores"])) for a, b in zip(dets, want)]
    d_plain = plain(x)
    assert not _same(dets, d_plain)
    view0 = ops.postprocess_logits(view_outputs[0], strides, anchors, plain.num_classes, thr, 1.0, 30000)   # every candidate of view 0 (its coarsest level included)
    foreign = 0
    for d, v0 in zip(dets, view0):
        have = {tuple(b) for b in v0["boxes"].cpu().numpy().tolist()}
        foreign += sum(tuple(b) not in have for b in d["boxes"].cpu().numpy().tolist())
    print("kept detections whose record comes from view 1 or 2:", foreign)
    assert foreign >= 1


# ---- 9. end to end against the restated pipeline, fp32 mode --------------------------------------------------------------------------------------------------------
def test_augment_fp32_mode_vs_the_restated_pipeline(dev):
    """views by torch (scale_img restated), the oracle's backbone and head per view, _descale_pred in float64, the concatenation without the tails, the oracle's NMS --
    against augment=True in fp32 mode; match_fraction with the thresholds of tests/test_e2e_gpu.py::test_yolov5s_640_vs_oracle"""
    from oracle import yolov5_oracle as O
    from test_e2e_gpu import _np, match_fraction
    thr = 0.1   # (on the CPU reference: 208 / 300 detections of 234 / 606 candidates, 25 / 76 of them more than the margin above the threshold; 0.25 leaves one)
    m = _core(dev, torch.float32, thr, augment=True)
    x = _batch(dev, torch.float32, n=2)
    dets = m.model(x)
    sd = {k[len("model."):]: v.float().cpu() for k, v in m.state_dict().items()}
    strides, anchors = O.anchors_for(3)
    with torch.no_grad():
        view_heads = [O.head(O.backbone(x.cpu() if r == 1.0 else T.scale_img_ref(x.cpu(), r, f), sd, "backbone"), sd, "head") for r, f in zip(T.SCALES, T.FLIPS)]
    xywh, conf = T.oracle_union(view_heads, CANVAS[1], strides, anchors)
    cands = T.union_candidates(xywh, conf, thr)
    import _merge_cases as M
    ref = M.merge_reference([(b.astype(np.float32), s, lab) for b, s, lab in cands], NMS, 300, False, False)
    for r, d in zip(ref, dets):
        r = {"boxes": r["boxes"].astype(np.float32), "scores": r["scores"], "labels": r["labels"]}
        frac, miou, ds = match_fraction(r, _np(d), margin=0.03, thr=thr)
        print(f"augment fp32 mode: {len(r['scores'])} ref dets, {len(d['scores'])} dets, matched {frac:.3f}, median IoU {miou:.4f}, max dscore {ds:.4f}")
        assert len(r["scores"]) > 10                      # the reference alone has enough detections above the threshold at this size
        assert frac >= 0.93 and miou >= 0.93, f"matched {frac:.3f} (max dscore {ds}) of {len(r['scores'])}"


# ---- 10. protocols -------------------------------------------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import test_tta_gpu as G
dev = torch.device("cuda:0")
m = G._core(dev, torch.float16, float(sys.argv[1]), augment=True)
print("CAP", m.model.cand_cap_per_image)
print("DETS " + G._pack(m.model(G._batch(dev, torch.float16))))
print("CAP", m.model.cand_cap_per_image)
"""


def _child(env_extra, thr):
    import base64
    import io
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests")), repr(thr)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("DETS ")][-1]
    caps = [int(l.split()[1]) for l in r.stdout.splitlines() if l.startswith("CAP ")]
    return [{k: v.to("cuda:0") for k, v in d.items()} for d in torch.load(io.BytesIO(base64.b64decode(line[5:])))], caps


PROTO_THR = 0.1


def test_capacity_growth_graphs_off_and_a_live_toggle(dev):
    x = _batch(dev, torch.float16)
    m = _core(dev, torch.float16, PROTO_THR, augment=True).model
    d_on = m(x)
    assert sum(len(d["scores"]) for d in d_on) > 20
    # a tiny candidate capacity grows and gives the same result
    got, caps = _child({"YOLORT_AMD_CAND_CAP": "64"}, PROTO_THR)
    assert caps[0] == 64 and caps[1] > 64 and _same(got, d_on), caps
    # per-kernel launches instead of the two captured graphs
    assert _same(_child({"YOLORT_AMD_GRAPH": "0"}, PROTO_THR)[0], d_on) and _same(_child({"YOLORT_AMD_POST_GRAPH": "0"}, PROTO_THR)[0], d_on)
    # the live attribute alternates between two plans
    d_off_ref = _core(dev, torch.float16, PROTO_THR).model(x)
    for _ in range(2):
        m.augment = False
        assert _same(m(x), d_off_ref)
        m.augment = True
        assert _same(m(x), d_on)
    assert not _same(d_on, d_off_ref) and len(m._ring) == 2
    # through YOLOv5 (letterbox of identity-size images: the planar-stem shortcut is off under augment, the canvas is filled)
    full = _core(dev, torch.float16, PROTO_THR, augment=True)
    assert _same(full.predict([im for im in x]), d_on)


def test_exported_plan_of_an_augmented_model_replays_identically(dev, tmp_path):
    from yolort_amd import _lib
    from yolort_amd._lib import PlanRegion, TAG_BOXES, TAG_INPUT, TAG_LABELS, TAG_RESCALE, TAG_SCORES, TAG_STATUS_COUNT
    lib = _lib.load(require_gpu=True)
    m = _core(dev, torch.float16, PROTO_THR, augment=True).model
    x = _batch(dev, torch.float16)
    dets = m(x)
    torch.cuda.synchronize()
    e = next(iter(m._entries.values()))
    path = str(tmp_path / "tta.ymiplan")
    info = m.export_plan(path, e.x.n, e.x.h, e.x.w, dev)
    plan2, regs, nreg = C.c_void_p(), (PlanRegion * 4096)(), C.c_int(0)
    assert lib.ymi_plan_import(path.encode(), C.byref(plan2), regs, 4096, C.byref(nreg)) == 0, lib.ymi_last_error()
    assert nreg.value == info["regions"]
    by_tag = {regs[i].tag: regs[i] for i in range(nreg.value) if regs[i].tag}
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int

    def read(tag, like):
        out = torch.empty_like(like)
        assert hip.hipMemcpy(out.data_ptr(), by_tag[tag].base, out.numel() * out.element_size(), 3) == 0
        return out

    try:
        torch.cuda.synchronize()
        for tag, src in ((TAG_INPUT, e.x.base), (TAG_RESCALE, e.rescale)):
            assert hip.hipMemcpy(by_tag[tag].base, src.data_ptr(), src.numel() * src.element_size(), 3) == 0
        s = torch.cuda.Stream()
        assert lib.ymi_plan_run(plan2, 0, -1, 0, C.c_void_p(s.cuda_stream)) == 0, lib.ymi_last_error()
        s.synchronize()
        boxes, scores, labels, sc = read(TAG_BOXES, e.post.boxes), read(TAG_SCORES, e.post.scores), read(TAG_LABELS, e.post.labels), read(TAG_STATUS_COUNT, e.post.status_count)
        torch.cuda.synchronize()
        cnt = sc[8:].tolist()
        assert sc[1].item() == 0 and cnt == [len(d["scores"]) for d in dets] and sum(cnt) > 20, (sc[:8].tolist(), cnt)
        for i, d in enumerate(dets):
            k = cnt[i]
            assert torch.equal(boxes[i, :k], d["boxes"]) and torch.equal(scores[i, :k], d["scores"]) and torch.equal(labels[i, :k], d["labels"])
    finally:
        lib.ymi_plan_destroy(plan2)
