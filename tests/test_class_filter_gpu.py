"""Class filter of the post-process (include/yolort_amd.h YMI_POST_CLASS_FILTER, `classes=[...]`) on the GPU: decode_kernel and the fused head's epilogue with the mask
against the reference of tests/_classes_cases.py (the oracle's decode, the filter as the header states it, the oracle's NMS), filtered against unfiltered runs bit for bit,
the capacity protocol on the filtered count, the global-sort path, the empty and the full set, a live model whose set changes between batches without a new plan, and an
exported plan that carries its set."""
import base64
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _agnostic_cases as A
import _classes_cases as K
import _head_cases as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -3.0
KEYS = ("count", "labels", "scores", "boxes")
CAP = 3 * 8192


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


def _flags(best, agnostic):
    return (K.POST_BEST_CLASS if best else 0) | (K.POST_AGNOSTIC if agnostic else 0)


# ---- whole post-process vs the reference ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("best", [False, True])
@pytest.mark.parametrize("nc", [2, 80])
def test_postprocess_class_filter_vs_reference(dev, nc, best, agnostic):
    """three images on levels (20, 24), (10, 12), (5, 6), runs (0.3, 300), (0.05, 7), (0.05, 300) with set A (nc = 2: (1,)), and (0.05, 300) with set B at nc = 80, under the
    host redo protocol: counts, labels, order exact; scores rtol 2e-6 / atol 1e-7, boxes rtol 1e-5 / atol 1e-4; slots past the count keep their fill; status[4] of the last
    pass = the candidates after the filter"""
    heads, strides, anchors, pred = A.post_inputs(nc, "full")
    runs = [(K.set_a(nc), thr, k) for thr, k in K.RUNS] + ([(K.SET_B, 0.05, 300)] if nc == 80 else [])
    for classes, thr, k in runs:
        ref = A.cut(K.full_ref(nc, False, thr, best, agnostic, classes), k)
        got = K.gpu_post(dev, heads, strides, anchors, nc, thr, k, CAP, _flags(best, agnostic), classes, fill=FILL)
        raw = sum(K.candidate_counts(pred, thr, best, classes))
        print(f"nc={nc} best={best} agnostic={agnostic} |set|={len(classes)} thr={thr} k={k}: detections {[len(r['scores']) for r in ref]} candidates {raw} "
              f"passes {[p[:5] for p in got['passes']]} cap {got['cap']}")
        H.assert_equals_oracle(got, ref, FILL)
        assert got["passes"][-1][4] == raw, (got["passes"], raw)
        for i in range(3):
            assert set(got["labels"][i, : int(got["count"][i])].tolist()) <= set(classes)


@pytest.mark.parametrize("best", [False, True])
def test_filtered_detections_are_the_allowed_subsequence_of_the_unfiltered_ones(dev, best):
    """class-aware NMS commutes with the filter (asserted from the oracle in tests/test_class_filter.py), so with k above the unfiltered survivor count and the exact full
    pass the filtered run's detections of an image are BIT-IDENTICAL to the unfiltered run's detections whose label is allowed: boxes, scores and labels -- the records of
    allowed classes are the unfiltered ones"""
    nc, thr, k = 80, 0.3, 8192
    heads, strides, anchors, _ = A.post_inputs(nc, "full")
    survivors = [len(r["scores"]) for r in A.post_full_ref(nc, "full", thr, best, False)]
    assert 0 < max(survivors) < k, survivors
    flags = _flags(best, False) | K.POST_EXACT_FULL
    plain = K.gpu_post(dev, heads, strides, anchors, nc, thr, k, CAP, flags, None, fill=FILL)
    for classes in (K.SET_A, K.SET_B):
        got = K.gpu_post(dev, heads, strides, anchors, nc, thr, k, CAP, flags, classes, fill=FILL)
        allowed = torch.tensor(sorted(classes))
        for i in range(3):
            c, cp = int(got["count"][i]), int(plain["count"][i])
            sel = torch.isin(plain["labels"][i, :cp], allowed)
            assert 0 < c == int(sel.sum()) < cp, (i, c, cp)
            for key in ("labels", "scores", "boxes"):
                assert torch.equal(got[key][i, :c], plain[key][i, :cp][sel]), (len(classes), i, key)


# ---- fused head on exact logits -----------------------------------------------------------------------------------------------------------------------------------------
# (case, set): set "A" = K.set_a(nc), "B" = its complement.  Chosen by what the case reaches UNDER the filter (asserted from the oracle's decode below):
#   worklist spill + record-buffer flush (more than 256 filtered records in one (run, anchor)): dense / B, nc60, nc92, nc123;  image change inside a wave: all of them;
#   padding channels (K % 32 != 0) at TNA = 1 ... 4: levels-4 (K = 16), nc28 (33), nc60 (65), nc92 (97);  no padding: nc27 (32), nc123 (128);  bf16: nc28-bfloat16
HEAD_RUNS = (("dense", "B"), ("nc27-float16", "A"), ("nc28-float16", "A"), ("nc60-float16", "A"), ("nc92-float16", "A"), ("nc123-float16", "A"), ("nc28-bfloat16", "B"),
             ("levels-4", "A"))
HEAD_SPILL = ("dense", "nc60-float16", "nc92-float16", "nc123-float16")
NA3_RUN = ("nc60-float16", "A")


def _head_set(name, which):
    nc = H.head_case(name)["nc"]
    a = K.set_a(nc)
    return a if which == "A" else tuple(c for c in range(nc) if c not in a)


def _assert_head_run_is_not_vacuous(name, classes, best):
    case = H.head_case(name)
    allowed = torch.zeros(case["nc"], dtype=torch.bool)
    allowed[list(classes)] = True
    filtered = dict(case, cand=case["cand"] & allowed)
    per_level, images = H.records_per_wave(filtered)
    densest = max(int(p.max()) for p in per_level)
    if name in HEAD_SPILL and not best:
        assert densest > max(H.HD_BUF_NA1, H.HD_WL_NA1), f"{name}: the densest filtered (run, anchor) has {densest} records"
    assert max(int(i.max()) for i in images) >= 2, f"{name}: no wave holds filtered candidates of two images"
    ref, plain = K.filtered_reference(case["pred"], case["thr"], case["nms"], case["k"], best, False, classes), K.filtered_reference(case["pred"], case["thr"], case["nms"], case["k"], best, False, None)
    assert any(A.differs(ref, plain)) and sum(len(r["scores"]) for r in ref) > 0
    return ref, densest


_HEAD_RESULTS = {}


def _head_forms(dev, name, which, best):
    key = (name, which, best)
    if key not in _HEAD_RESULTS:
        case, classes = H.head_case(name), _head_set(name, which)
        _HEAD_RESULTS[key] = {mode: K.gpu_head(dev, case, mode, classes, K.POST_BEST_CLASS if best else 0, FILL) for mode in H.HEAD_MODES}
    return _HEAD_RESULTS[key]


@pytest.mark.parametrize("name,which", HEAD_RUNS)
def test_fused_head_class_filter_on_exact_logits(dev, name, which):
    """group launch, per-level launches and the stored-logits post-process of a case with a class set: the fused result equals the filtered reference, the three forms
    agree bit for bit, status[4] = the filtered candidate count"""
    case, classes = H.head_case(name), _head_set(name, which)
    ref, densest = _assert_head_run_is_not_vacuous(name, classes, False)
    raw = sum(K.candidate_counts(case["pred"], case["thr"], False, classes))
    got = _head_forms(dev, name, which, False)
    print(f"{name} / {which}: {len(classes)} of {case['nc']} classes, candidates {raw} of {sum(case['candidates_per_image'])}, densest filtered (run, anchor) {densest}, "
          f"passes {got['group']['passes']}")
    H.assert_equals_oracle(got["group"], ref, FILL)
    for mode in H.HEAD_MODES:
        assert got[mode]["passes"][-1][4] == raw, (mode, got[mode]["passes"], raw)
    for mode in ("single", "unfused"):
        for key in KEYS:
            assert torch.equal(got[mode][key], got["group"][key]), f"{mode} differs from the group launch in {key}"
        assert got[mode]["passes"][-1][0] == got["group"]["passes"][-1][0]


@pytest.mark.parametrize("name,which", [("nc60-float16", "A"), ("dense", "B"), ("nc28-bfloat16", "B")])
def test_fused_head_class_filter_best_class_on_exact_logits(dev, name, which):
    """the same in best-class mode: the winner is taken over all classes, its record is written only if it is allowed"""
    case, classes = H.head_case(name), _head_set(name, which)
    ref, _ = _assert_head_run_is_not_vacuous(name, classes, True)
    misread = K.filtered_reference(case["pred"], case["thr"], case["nms"], case["k"], True, False, classes, "before", "allowed-argmax")
    raw = sum(K.candidate_counts(case["pred"], case["thr"], True, classes))
    got = _head_forms(dev, name, which, True)
    print(f"{name} / {which}: passing anchors with an allowed best class {raw}; differs from argmax over the allowed classes: {A.differs(ref, misread)}")
    H.assert_equals_oracle(got["group"], ref, FILL)
    for mode in H.HEAD_MODES:
        assert got[mode]["passes"][-1][4] == raw, (mode, got[mode]["passes"], raw)
        for key in KEYS:
            assert torch.equal(got[mode][key], got["group"][key]), f"{mode} differs from the group launch in {key}"


_CHILD = r"""
import base64, io, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import _classes_cases as K, _head_cases as H
dev = torch.device("cuda:0")
name, classes = sys.argv[1], tuple(int(c) for c in sys.argv[2].split(","))
case = H.head_case(name)
for best in (0, 1):
    for mode in ("group", "single"):
        got = K.gpu_head(dev, case, mode, classes, K.POST_BEST_CLASS if best else 0, %r)
        buf = io.BytesIO()
        np.savez_compressed(buf, **{k: got[k].numpy() for k in ("count", "labels", "scores", "boxes")})
        print("DET", best, mode, base64.b64encode(buf.getvalue()).decode(), flush=True)
print("DONE")
"""


def test_three_anchors_per_wave_honour_the_filter(dev):
    """YOLORT_AMD_HEAD_SPLIT=0 (read once per process: a fresh child process) selects the NA = 3 instantiations: nc = 60 (TNA = 3, padding rows) with set A, both candidate
    modes, both launches -- equal to the reference and to this process's NA = 1 results bit for bit"""
    name, which = NA3_RUN
    classes = _head_set(name, which)
    case = H.head_case(name)
    env = dict(os.environ, YOLORT_AMD_HEAD_SPLIT="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), FILL), name, ",".join(map(str, classes))], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("DONE"), (r.returncode, r.stderr[-3000:])
    seen = set()
    for line in r.stdout.splitlines():
        if not line.startswith("DET "):
            continue
        _, best, mode, blob = line.split(" ", 3)
        best = bool(int(best))
        z = np.load(io.BytesIO(base64.b64decode(blob)))
        got = {k: torch.from_numpy(z[k]) for k in KEYS}
        H.assert_equals_oracle(got, K.filtered_reference(case["pred"], case["thr"], case["nms"], case["k"], best, False, classes), FILL)
        mine = _head_forms(dev, name, which, best)["group"]
        for key in KEYS:
            assert torch.equal(got[key], mine[key]), f"best={best} / {mode}: NA = 3 differs from NA = 1 in {key}"
        seen.add((best, mode))
    assert seen == {(b, m) for b in (False, True) for m in ("group", "single")}, seen


# ---- capacity, global sort, edges -------------------------------------------------------------------------------------------------------------------------------------------
def test_a_filtered_batch_that_fits_its_capacity_is_not_redone(dev):
    """the capacity protocol counts the FILTERED records: a capacity between the largest filtered and the largest unfiltered per-image count (from the oracle) holds the
    filtered batch in one pass -- status[1] == 0, status[4] = the oracle's filtered count -- while the unfiltered batch overflows it"""
    nc, thr, k, classes = 80, 0.05, 300, K.SET_A
    heads, strides, anchors, pred = A.post_inputs(nc, "full")
    filt, unf = K.candidate_counts(pred, thr, False, classes), K.candidate_counts(pred, thr, False, None)
    cap_img = 1 << (max(filt) - 1).bit_length()   # per-image regions are powers of two
    print(f"filtered {filt}, unfiltered {unf}, capacity per image {cap_img}")
    assert 64 <= max(filt) <= cap_img < max(unf)
    got = K.gpu_post(dev, heads, strides, anchors, nc, thr, k, 3 * cap_img, 0, classes, fill=FILL, one_pass=True)
    st = got["passes"][0]
    assert st[1] == 0 and st[4] == sum(filt), st
    H.assert_equals_oracle(got, A.cut(K.full_ref(nc, False, thr, False, False, classes), k), FILL)
    plain = K.gpu_post(dev, heads, strides, anchors, nc, thr, k, 3 * cap_img, 0, None, fill=FILL, one_pass=True)
    assert plain["passes"][0][1] & 1, plain["passes"]


@pytest.mark.parametrize("best", [False, True])
def test_global_sort_path_with_a_class_set(dev, best):
    """cand_cap / n < 64: the global candidate list and the radix sort; 64 images, nc = 3, classes (0, 2); one pass"""
    g, classes = A.GLOBAL, (0, 2)
    heads, strides, anchors, pred = A.global_inputs(64)
    ref = K.filtered_reference(pred, g["thr"], 0.45, g["k"], best, False, classes)
    plain = K.filtered_reference(pred, g["thr"], 0.45, g["k"], best, False, None)
    assert sum(A.differs(ref, plain)) >= 32 and sum(len(r["scores"]) for r in ref) > 64
    got = K.gpu_post(dev, heads, strides, anchors, g["nc"], g["thr"], g["k"], 64 * g["per_image_cap"], _flags(best, False), classes, fill=FILL)
    assert len(got["passes"]) == 1 and got["passes"][0][1] == 0 and got["cap"] == 64 * g["per_image_cap"], got["passes"]
    assert got["passes"][0][4] == sum(K.candidate_counts(pred, g["thr"], best, classes))
    H.assert_equals_oracle(got, ref, FILL)


def test_the_empty_set_and_the_full_set(dev):
    """classes=[]: zero detections in every image, the slab's count column 0 (not the stale marker), nothing else written; classes=range(nc): bit-identical to no filter"""
    nc, thr, k = 80, 0.3, 300
    heads, strides, anchors, _ = A.post_inputs(nc, "full")
    for best in (False, True):
        none = K.gpu_post(dev, heads, strides, anchors, nc, thr, k, CAP, _flags(best, False), (), fill=FILL)
        assert none["count"].tolist() == [0, 0, 0] and none["passes"][-1][1] == 0 and none["passes"][-1][4] == 0 and none["passes"][-1][0] == 0, none["passes"]
        assert (none["slab"][:, -1] == 0).all() and (none["slab"][:, :-1] == 0).all(), "the slab of an empty result: count 0, slots zeroed"
        assert (none["scores"] == FILL).all() and (none["boxes"] == FILL).all()
        plain = K.gpu_post(dev, heads, strides, anchors, nc, thr, k, CAP, _flags(best, False), None, fill=FILL)
        full = K.gpu_post(dev, heads, strides, anchors, nc, thr, k, CAP, _flags(best, False), range(nc), fill=FILL)
        assert int(plain["count"].sum()) > 0
        for key in KEYS + ("slab",):
            assert torch.equal(plain[key], full[key]), (best, key)
        assert [p[1] for p in plain["passes"]] == [p[1] for p in full["passes"]] and plain["passes"][-1] == full["passes"][-1]


def test_python_validation_on_the_device_path(dev):
    from yolort_amd.ops import postprocess_logits
    heads, strides, anchors, _ = A.post_inputs(2, "full")
    with pytest.raises(ValueError):
        postprocess_logits([h.to(dev) for h in heads], strides, anchors, 2, 0.3, 0.45, 300, classes=[2])
    got = postprocess_logits([h.to(dev) for h in heads], strides, anchors, 2, 0.3, 0.45, 300, classes=[1, 1])
    ref = A.cut(K.full_ref(2, False, 0.3, False, False, (1,)), 300)
    assert [len(d["scores"]) for d in got] == [len(r["scores"]) for r in ref] and all(torch.equal(d["labels"].cpu(), r["labels"]) for d, r in zip(got, ref))


# ---- whole model --------------------------------------------------------------------------------------------------------------------------------------------------------
ARCH, NC = "yolov5_darknet_pan_n_r60", 80


def _model(dev, **kw):
    from yolort_amd.models import YOLOv5
    from workloads.synth import synth_weights
    m = YOLOv5(arch=ARCH, score_thresh=0.05, nms_thresh=0.45, **kw)
    m.load_state_dict(synth_weights(m.state_dict(), ARCH, seed=0, head_gain=0.8))
    return m.to(dev).half().eval()


def _batch(dev, seed=5):
    from workloads.synth import synth_images
    return torch.stack([im for im in synth_images(2, 128, 128, seed=seed)]).to(dev).half()


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("boxes", "scores", "labels"))


def _labels(dets):
    return set(int(v) for d in dets for v in d["labels"].tolist())


@pytest.mark.parametrize("fused", [True, False])
def test_changing_the_set_on_a_live_model_needs_no_new_plan(dev, fused):
    """yolov5n, two 128 x 128 images: post_process.classes = A, then B, then None -- each takes effect on the next batch and equals a freshly constructed model; between A
    and B the plan rings and the entry's plan object are the same (the set is data in the plan's workspace); A -> None selects another plan"""
    m, x = _model(dev), _batch(dev)
    core = m.model
    core.fuse_head_decode = fused
    core.post_process.classes = K.SET_A
    d_a = core(x)
    e_a = next(iter(core._entries.values()))
    rings, plan_a = len(core._ring), e_a.plan
    assert e_a.mask_classes == K.SET_A and (e_a.logits is None) == fused
    core.post_process.classes = K.SET_B
    d_b = core(x)
    e_b = next(iter(core._entries.values()))
    assert len(core._ring) == rings and e_b is e_a and e_b.plan is plan_a and e_b.mask_classes == K.SET_B, "a new set must not build a new plan"
    core.post_process.classes = K.SET_A
    assert _same(core(x), d_a) and len(core._ring) == rings
    core.post_process.classes = None
    d_none = core(x)
    e_none = next(iter(core._entries.values()))
    assert len(core._ring) == rings + 1 and e_none.plan is not plan_a
    print("detections A", [len(d["scores"]) for d in d_a], "B", [len(d["scores"]) for d in d_b], "none", [len(d["scores"]) for d in d_none])
    assert sum(len(d["scores"]) for d in d_a) > 0 and _labels(d_a) <= set(K.SET_A) and _labels(d_b) <= set(K.SET_B) and _labels(d_b)
    assert not _same(d_a, d_b) and not _same(d_a, d_none) and not _same(d_b, d_none)
    for classes, want in ((K.SET_A, d_a), (K.SET_B, d_b), (None, d_none)):
        ref = _model(dev, classes=classes)
        ref.model.fuse_head_decode = fused
        assert _same(ref.model(x), want), f"live model and a fresh model disagree for {classes}"
    core.post_process.classes = [NC]
    with pytest.raises(ValueError):
        core(x)


def test_batches_in_flight_are_filtered_by_their_own_set(dev):
    """pipeline_depth > 1: two batches submitted back to back with different sets (and a third with the first set again) each come back filtered by the set they were
    submitted under"""
    m, x, y = _model(dev), _batch(dev), _batch(dev, seed=6)
    core = m.model
    assert core.pipeline_depth > 1
    want = {}
    for classes in (K.SET_A, K.SET_B):
        ref = _model(dev, classes=classes)
        want[classes] = (ref.model(x), ref.model(y))
    core.post_process.classes = K.SET_A
    p1 = core.submit(x)
    core.post_process.classes = K.SET_B
    p2 = core.submit(y)
    p3 = core.submit(x)
    core.post_process.classes = K.SET_A
    p4 = core.submit(y)
    r1, r2, r3, r4 = p1.result(), p2.result(), p3.result(), p4.result()
    assert _same(r1, want[K.SET_A][0]) and _same(r2, want[K.SET_B][1]) and _same(r3, want[K.SET_B][0]) and _same(r4, want[K.SET_A][1])
    assert sum(len(d["scores"]) for d in r1) > 0 and not _same(r1, r3)


def test_exported_plan_carries_its_class_set(dev, tmp_path):
    """export with a filter; import and replay through the C ABI alone, without calling anything else: the result is the model's filtered one bit for bit; then
    ymi_plan_set_classes with set B: the replay equals a model filtered by B"""
    import ctypes as C
    from yolort_amd import _lib
    from yolort_amd._lib import PlanRegion, TAG_BOXES, TAG_INPUT, TAG_LABELS, TAG_RESCALE, TAG_SCORES, TAG_STATUS_COUNT
    from workloads.synth import synth_images
    lib = _lib.load(require_gpu=True)
    S = 160
    m = _model(dev, classes=K.SET_A, size=(S, S))
    imgs = [synth_images(1, S - 40, S, seed=21)[0].to(dev).half(), synth_images(1, S, S - 64, seed=22)[0].to(dev).half()]
    dets = m.predict(imgs)
    torch.cuda.synchronize()
    e = next(iter(m.model._entries.values()))
    path = str(tmp_path / "classes.ymiplan")
    info = m.model.export_plan(path, e.x.n, e.x.h, e.x.w, dev)
    m.model.post_process.classes = K.SET_B
    dets_b = m.predict(imgs)
    m.model.post_process.classes = None
    dets_none = m.predict(imgs)
    assert sum(len(d["scores"]) for d in dets) > 0 and _labels(dets) <= set(K.SET_A) and not _same(dets, dets_b) and not _same(dets, dets_none)
    plan2, regs, nreg = C.c_void_p(), (PlanRegion * 4096)(), C.c_int(0)
    assert lib.ymi_plan_import(path.encode(), C.byref(plan2), regs, 4096, C.byref(nreg)) == 0, lib.ymi_last_error()
    assert nreg.value == info["regions"]
    by_tag = {regs[i].tag: regs[i] for i in range(nreg.value) if regs[i].tag}
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int

    def dev_copy(dst_ptr, src):
        torch.cuda.synchronize()
        assert hip.hipMemcpy(dst_ptr, src.data_ptr(), src.numel() * src.element_size(), 3) == 0

    def read(tag, like):
        out = torch.empty_like(like)
        assert hip.hipMemcpy(out.data_ptr(), by_tag[tag].base, out.numel() * out.element_size(), 3) == 0
        return out

    def replay_equals(want):
        s = torch.cuda.Stream()
        assert lib.ymi_plan_run(plan2, 0, -1, 0, C.c_void_p(s.cuda_stream)) == 0, lib.ymi_last_error()
        s.synchronize()
        boxes, scores, labels, sc = read(TAG_BOXES, e.post.boxes), read(TAG_SCORES, e.post.scores), read(TAG_LABELS, e.post.labels), read(TAG_STATUS_COUNT, e.post.status_count)
        torch.cuda.synchronize()
        cnt = sc[8:].tolist()
        assert sc[1].item() == 0 and cnt == [len(d["scores"]) for d in want], (sc[:8].tolist(), cnt, [len(d["scores"]) for d in want])
        for i, d in enumerate(want):
            k = cnt[i]
            assert torch.equal(boxes[i, :k], d["boxes"]) and torch.equal(scores[i, :k], d["scores"]) and torch.equal(labels[i, :k], d["labels"])

    try:
        dev_copy(by_tag[TAG_INPUT].base, e.x.base)
        dev_copy(by_tag[TAG_RESCALE].base, e.rescale)
        replay_equals(dets)
        arr = (C.c_int32 * len(K.SET_B))(*K.SET_B)
        assert lib.ymi_plan_set_classes(plan2, arr, len(K.SET_B), None) == 0, lib.ymi_last_error()
        torch.cuda.synchronize()
        replay_equals(dets_b)
        bad = (C.c_int32 * 1)(NC)
        assert lib.ymi_plan_set_classes(plan2, bad, 1, None) == -1 and b"class index" in lib.ymi_last_error()
    finally:
        lib.ymi_plan_destroy(plan2)


def _replay_imported(path, regions, e, want):
    """imports the plan file, feeds it the entry's canvas and rescale rows, replays it once through the C ABI and compares the detection arrays with `want` bit for bit"""
    import ctypes as C
    from yolort_amd import _lib
    from yolort_amd._lib import PlanRegion, TAG_BOXES, TAG_INPUT, TAG_LABELS, TAG_RESCALE, TAG_SCORES, TAG_STATUS_COUNT
    lib = _lib.load(require_gpu=True)
    plan2, regs, nreg = C.c_void_p(), (PlanRegion * 4096)(), C.c_int(0)
    assert lib.ymi_plan_import(path.encode(), C.byref(plan2), regs, 4096, C.byref(nreg)) == 0, lib.ymi_last_error()
    try:
        assert nreg.value == regions
        by_tag = {regs[i].tag: regs[i] for i in range(nreg.value) if regs[i].tag}
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
        torch.cuda.synchronize()
        for tag, src in ((TAG_INPUT, e.x.base), (TAG_RESCALE, e.rescale)):
            assert hip.hipMemcpy(by_tag[tag].base, src.data_ptr(), src.numel() * src.element_size(), 3) == 0
        s = torch.cuda.Stream()
        assert lib.ymi_plan_run(plan2, 0, -1, 0, C.c_void_p(s.cuda_stream)) == 0, lib.ymi_last_error()
        s.synchronize()
        got = {}
        for tag, like in ((TAG_BOXES, e.post.boxes), (TAG_SCORES, e.post.scores), (TAG_LABELS, e.post.labels), (TAG_STATUS_COUNT, e.post.status_count)):
            got[tag] = torch.empty_like(like)
            assert hip.hipMemcpy(got[tag].data_ptr(), by_tag[tag].base, like.numel() * like.element_size(), 3) == 0
        torch.cuda.synchronize()
        sc = got[TAG_STATUS_COUNT]
        cnt = sc[8:].tolist()
        assert sc[1].item() == 0 and cnt == [len(d["scores"]) for d in want], (sc[:8].tolist(), cnt, [len(d["scores"]) for d in want])
        for i, d in enumerate(want):
            k = cnt[i]
            assert torch.equal(got[TAG_BOXES][i, :k], d["boxes"]) and torch.equal(got[TAG_SCORES][i, :k], d["scores"]) and torch.equal(got[TAG_LABELS][i, :k], d["labels"])
    finally:
        lib.ymi_plan_destroy(plan2)


def test_export_writes_the_set_the_model_has_now(dev, tmp_path):
    """export_plan BEFORE the first batch (the plan instance has never run: nothing has written its mask yet), and again after post_process.classes changed with no batch in
    between (the instance last ran under the other set): either file filters as the model does at the moment of the export"""
    from workloads.synth import synth_images
    S = 160
    m = _model(dev, classes=K.SET_A, size=(S, S))
    core = m.model
    path_a, path_b = str(tmp_path / "first.ymiplan"), str(tmp_path / "changed.ymiplan")
    info_a = core.export_plan(path_a, 2, S, S, dev)
    imgs = [synth_images(1, S - 40, S, seed=21)[0].to(dev).half(), synth_images(1, S, S - 64, seed=22)[0].to(dev).half()]
    dets_a = m.predict(imgs)
    torch.cuda.synchronize()
    e = next(iter(core._entries.values()))
    assert (e.x.n, e.x.h, e.x.w) == (2, S, S) and len(core._ring) == 1, "the exported plan is not the one the batch ran on"
    assert sum(len(d["scores"]) for d in dets_a) > 0 and _labels(dets_a) <= set(K.SET_A)
    _replay_imported(path_a, info_a["regions"], e, dets_a)
    core.post_process.classes = K.SET_B
    info_b = core.export_plan(path_b, 2, S, S, dev)            # every instance of the ring last ran under set A
    dets_b = m.predict(imgs)
    torch.cuda.synchronize()
    assert len(core._ring) == 1 and _labels(dets_b) <= set(K.SET_B) and _labels(dets_b) and not _same(dets_a, dets_b)
    _replay_imported(path_b, info_b["regions"], next(iter(core._entries.values())), dets_b)


def test_a_redo_runs_under_the_set_the_batch_was_submitted_with(dev):
    """pipeline_depth > 1, a candidate capacity that the batch overflows: the batch is submitted under set B, post_process.classes then becomes A (and, in a second round,
    None -- another plan key); result() has to grow the capacity and re-run the batch, and the re-run is filtered by B; the live attribute stays what the caller set"""
    m, x = _model(dev), _batch(dev)
    core = m.model
    assert core.pipeline_depth > 1
    want = _model(dev, classes=K.SET_B).model(x)
    assert sum(len(d["scores"]) for d in want) > 0
    for later in (K.SET_A, None):
        core.cand_cap_per_image = 64                      # below the filtered candidate count of an image: the first pass overflows (nothing is truncated)
        core.post_process.classes = K.SET_B
        p = core.submit(x)
        core.post_process.classes = later
        got = p.result()
        assert core.cand_cap_per_image > 64, "the batch was not redone: the test shows nothing"
        assert core.post_process.classes == later
        assert _same(got, want), f"the re-run was not filtered by the submitted set (live attribute: {later})"
