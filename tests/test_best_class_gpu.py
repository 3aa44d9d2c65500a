"""Best-class post-process mode (include/yolort_amd.h YMI_POST_BEST_CLASS, `multi_label=False`) on the GPU: decode_kernel (postprocess.hip) and the fused head's epilogue
(head_decode.hpp) through the group launch, the per-level launches and the stored-logits post-process, against the restated reference of tests/_best_cases.py on inputs
whose logits are exact, against each other bit for bit, the NA = 3 instantiations in a fresh child process, and a whole model: fused = unfused = ops.postprocess_logits,
the fp32 parity mode, the mode flipped on a live model, an exported plan."""
import base64
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _best_cases as B
import _head_cases as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -3.0
KEYS = ("count", "labels", "scores", "boxes")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


_RESULTS = {}


def _forms(dev, name):
    """the three forms of a case in best-class mode (shared by the tests that need them, left unchanged)"""
    if name not in _RESULTS:
        case = B.best_case(name)
        _RESULTS[name] = {mode: B.gpu_best(dev, case, mode, B.POST_BEST_CLASS, FILL) for mode in H.HEAD_MODES}
    return _RESULTS[name]


@pytest.mark.parametrize("name", B.EXISTING + B.NEW_CASES)
def test_best_class_equals_the_reference_on_exact_logits(dev, name):
    """group launch, per-level launches and the stored-logits post-process of one case, all with YMI_POST_BEST_CLASS: the group launch equals the restated reference
    (counts, labels, order exact; scores rtol 2e-6 / atol 1e-7, boxes rtol 1e-5 / atol 1e-4; slots past the count keep their fill), and the three forms agree bit for
    bit -- counts, labels, scores, boxes (torch.equal) and status[4], the number of passing anchors."""
    print(B.assert_best_case_is_not_vacuous(name))
    case, ref = B.best_case(name), B.best_reference(name)
    got = _forms(dev, name)
    for mode in H.HEAD_MODES:
        print(mode, "passes", got[mode]["passes"], "cap", got[mode]["cap"])
    H.assert_equals_oracle(got["group"], ref, FILL)
    conf = (case["pred"][..., 5:] * case["pred"][..., 4:5]).max(-1).values
    passing = int((conf > case["thr"]).sum())
    for mode in H.HEAD_MODES:
        assert got[mode]["passes"][-1][4] == passing, (mode, got[mode]["passes"], passing)
    for mode in ("single", "unfused"):
        for key in KEYS:
            assert torch.equal(got[mode][key], got["group"][key]), f"{mode} differs from the group launch in {key}"
        assert got[mode]["cap"] == got["group"]["cap"]
    if case["exact"] and case["design"] in ("palette", "best"):
        for i in range(case["n"]):
            s = got["group"]["scores"][i, : int(got["group"]["count"][i])]
            assert torch.isin(s, torch.tensor(case["exact"])).all() and bool((s > case["thr"]).all()), s
    if name in B.NEW_SPECS and case["expect_candidates"] is not None:
        assert int(got["group"]["count"].sum()) == case["expect_candidates"]


def test_one_class_is_bit_identical_to_the_default_mode(dev):
    """num_classes == 1: the best class is the only class -- every form equals the flag-less run bit for bit, status words included"""
    case = B.best_case("one-class")
    for mode in H.HEAD_MODES:
        plain = B.gpu_best(dev, case, mode, 0, FILL)
        best = _forms(dev, "one-class")[mode]
        for key in KEYS:
            assert torch.equal(plain[key], best[key]), (mode, key)
        assert plain["passes"] == best["passes"], (mode, plain["passes"], best["passes"])
    assert int(plain["count"].sum()) > 0


_CHILD = r"""
import base64, io, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import _best_cases as B
dev = torch.device("cuda:0")
for name in sys.argv[1:]:
    case = B.best_case(name)
    for mode in ("group", "single"):
        got = B.gpu_best(dev, case, mode, B.POST_BEST_CLASS, %r)
        buf = io.BytesIO()
        np.savez_compressed(buf, **{k: got[k].numpy() for k in ("count", "labels", "scores", "boxes")})
        print("DET", name, mode, base64.b64encode(buf.getvalue()).decode(), flush=True)
print("DONE")
"""


def test_three_anchors_per_wave_in_best_class_mode(dev):
    """YOLORT_AMD_HEAD_SPLIT=0 (read once per process: a fresh child) selects the NA = 3 instantiations: the ties, the padding cases and one class count per TNA through
    both launches with YMI_POST_BEST_CLASS.  The child prints its detections; they equal the reference and this process's NA = 1 results bit for bit."""
    assert {(B.best_case(nm)["nc"] + 36) // 32 for nm in B.NA3_CASES} >= {1, 2, 3, 4}
    env = dict(os.environ, YOLORT_AMD_HEAD_SPLIT="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), FILL), *B.NA3_CASES], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("DONE"), (r.returncode, r.stderr[-3000:])
    seen = set()
    for line in r.stdout.splitlines():
        if not line.startswith("DET "):
            continue
        _, name, mode, blob = line.split(" ", 3)
        z = np.load(io.BytesIO(base64.b64decode(blob)))
        got = {k: torch.from_numpy(z[k]) for k in KEYS}
        H.assert_equals_oracle(got, B.best_reference(name), FILL)
        mine = _forms(dev, name)["group"]
        for key in KEYS:
            assert torch.equal(got[key], mine[key]), f"{name} / {mode}: NA = 3 differs from NA = 1 in {key}"
        seen.add((name, mode))
    assert seen == {(name, mode) for name in B.NA3_CASES for mode in ("group", "single")}, seen


# ---- whole model -------------------------------------------------------------------------------------------------------------------------------------------------------
ARCH, NC = "yolov5_darknet_pan_n_r60", 80


def _model(dev, dtype=torch.float16, **kw):
    from yolort_amd.models import YOLOv5
    from workloads.synth import synth_weights
    m = YOLOv5(arch=ARCH, score_thresh=0.1, nms_thresh=0.45, **kw)
    m.load_state_dict(synth_weights(m.state_dict(), ARCH, seed=0, head_gain=0.8))
    return m.to(dev).to(dtype).eval()


def _batch(dev, dtype=torch.float16):
    from workloads.synth import synth_images
    return torch.stack([im for im in synth_images(2, 96, 128, seed=5)]).to(dev).to(dtype)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("boxes", "scores", "labels"))


def test_whole_model_fused_unfused_and_postprocess_logits_agree(dev):
    """yolov5n with seeded weights on two 3 x 96 x 128 images, multi_label=False: the fused head equals the stored-logits form bit for bit, and both equal
    ops.postprocess_logits(head outputs, multi_label=False); no anchor is detected twice; the default mode returns more (the same anchors under several labels)"""
    from yolort_amd.ops import postprocess_logits
    m, x = _model(dev, multi_label=False), _batch(dev)
    assert m.model.post_process.multi_label is False and m.model.fuse_head_decode
    fused = m.model(x)
    e = next(iter(m.model._entries.values()))
    assert e.logits is None
    passing = int(e.post.status[4].item())
    m.model.fuse_head_decode = False
    unfused = m.model(x)
    e = next(iter(m.model._entries.values()))
    assert e.logits is not None and int(e.post.status[4].item()) == passing
    assert _same(fused, unfused), "fused / unfused head disagree in best-class mode"
    heads = []
    for v in e.logits:
        t = v.as_tensor()
        heads.append(t.reshape(t.shape[0], t.shape[1], t.shape[2], 3, NC + 5).permute(0, 3, 1, 2, 4).contiguous())
    ag, pp = m.model.anchor_generator, m.model.post_process
    args = (heads, [float(s) for s in ag.strides], ag.anchor_grids, NC, float(pp.score_thresh), float(pp.nms_thresh), int(pp.detections_per_img))
    want = postprocess_logits(*args, multi_label=False)
    assert _same(unfused, want), "model / postprocess_logits disagree in best-class mode"
    n_det = [len(d["scores"]) for d in fused]
    print("detections", n_det, "passing anchors", passing)
    assert sum(n_det) > 10 and 0 < passing <= 2 * sum(3 * v.h * v.w for v in e.logits)
    multi = postprocess_logits(*args)
    assert sum(len(d["scores"]) for d in multi) > sum(n_det) or int(pp.detections_per_img) in [len(d["scores"]) for d in multi]
    assert not _same(multi, want)


def test_toggling_multi_label_on_a_live_model_takes_effect_on_the_next_batch(dev):
    """no stale plan: the detections change with `post_process.multi_label` and change back, with the fused and with the unfused head"""
    m, x = _model(dev), _batch(dev)
    for fused in (True, False):
        m.model.fuse_head_decode = fused
        m.model.post_process.multi_label = True
        multi = m.model(x)
        m.model.post_process.multi_label = False
        best = m.model(x)
        e = next(iter(m.model._entries.values()))
        assert int(e.post.status[4].item()) <= 2 * e.post.total_anchors
        m.model.post_process.multi_label = True
        again = m.model(x)
        assert _same(multi, again) and not _same(multi, best), fused
        ref = _model(dev, multi_label=False)
        ref.model.fuse_head_decode = fused
        assert _same(best, ref.model(x)), fused


def test_fp32_parity_mode_agrees_on_labels_and_counts(dev):
    """the fp32 parity mode (exact fp32 convolutions, stored logits, decode_kernel) runs in best-class mode and agrees with ops.postprocess_logits(its own logits,
    multi_label=False) on labels and counts (and on everything else: the same kernel); how it compares with the fp16 model is printed"""
    from yolort_amd.ops import postprocess_logits
    x = _batch(dev)
    d16 = _model(dev, multi_label=False).model(x)
    m32 = _model(dev, torch.float32, multi_label=False)
    m32.set_compute_dtype(torch.float32)
    d32 = m32.model(x.float())
    e = next(iter(m32.model._entries.values()))
    assert e.logits is not None, "the parity mode keeps the fp32 logits"
    heads = []
    for v in e.logits:
        t = v.as_tensor()
        heads.append(t.reshape(t.shape[0], t.shape[1], t.shape[2], 3, NC + 5).permute(0, 3, 1, 2, 4).contiguous())
    ag, pp = m32.model.anchor_generator, m32.model.post_process
    want = postprocess_logits(heads, [float(s) for s in ag.strides], ag.anchor_grids, NC, float(pp.score_thresh), float(pp.nms_thresh), int(pp.detections_per_img), multi_label=False)
    assert sum(len(d["scores"]) for d in d32) > 10
    for d, r in zip(d32, want):
        assert len(d["scores"]) == len(r["scores"]) and torch.equal(d["labels"], r["labels"])
    assert _same(d32, want)
    for a, b in zip(d16, d32):
        print("fp16", len(a["scores"]), "fp32", len(b["scores"]), "detections; labels in common", len(set(a["labels"].tolist()) & set(b["labels"].tolist())))


def test_exported_plan_with_the_flag_replays_to_the_same_detections(dev, tmp_path):
    """the descriptor travels with the plan: an exported best-class plan, replayed through the C ABI alone, returns the model's detections bit for bit"""
    import ctypes as C
    from yolort_amd import _lib
    from yolort_amd._lib import PlanRegion, TAG_BOXES, TAG_INPUT, TAG_LABELS, TAG_RESCALE, TAG_SCORES, TAG_STATUS_COUNT
    from workloads.synth import synth_images
    lib = _lib.load(require_gpu=True)
    S = 160
    m = _model(dev, multi_label=False, size=(S, S))
    imgs = [synth_images(1, S - 40, S, seed=21)[0].to(dev).half(), synth_images(1, S, S - 64, seed=22)[0].to(dev).half()]
    dets = m.predict(imgs)
    torch.cuda.synchronize()
    m.model.post_process.multi_label = True
    multi = m.predict(imgs)
    m.model.post_process.multi_label = False
    assert sum(len(d["scores"]) for d in dets) > 0 and not _same(dets, multi)
    dets2 = m.predict(imgs)
    assert _same(dets, dets2)
    e = next(iter(m.model._entries.values()))
    path = str(tmp_path / "best.ymiplan")
    info = m.model.export_plan(path, e.x.n, e.x.h, e.x.w, dev)
    plan2, regs, nreg = C.c_void_p(), (PlanRegion * 4096)(), C.c_int(0)
    assert lib.ymi_plan_import(path.encode(), C.byref(plan2), regs, 4096, C.byref(nreg)) == 0, lib.ymi_last_error()
    assert nreg.value == info["regions"]
    by_tag = {regs[i].tag: regs[i] for i in range(nreg.value) if regs[i].tag}
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int

    def dev_copy(dst_ptr, src):
        torch.cuda.synchronize()
        assert hip.hipMemcpy(dst_ptr, src.data_ptr(), src.numel() * src.element_size(), 3) == 0

    dev_copy(by_tag[TAG_INPUT].base, e.x.base)
    dev_copy(by_tag[TAG_RESCALE].base, e.rescale)
    s = torch.cuda.Stream()
    assert lib.ymi_plan_run(plan2, 0, -1, 0, C.c_void_p(s.cuda_stream)) == 0, lib.ymi_last_error()
    s.synchronize()

    def read(tag, like):
        out = torch.empty_like(like)
        assert hip.hipMemcpy(out.data_ptr(), by_tag[tag].base, out.numel() * out.element_size(), 3) == 0
        return out

    boxes, scores, labels, sc = read(TAG_BOXES, e.post.boxes), read(TAG_SCORES, e.post.scores), read(TAG_LABELS, e.post.labels), read(TAG_STATUS_COUNT, e.post.status_count)
    torch.cuda.synchronize()
    cnt = sc[8:].tolist()
    assert cnt == [len(d["scores"]) for d in dets], (cnt, [len(d["scores"]) for d in dets])
    for i, d in enumerate(dets):
        k = cnt[i]
        assert torch.equal(boxes[i, :k], d["boxes"]) and torch.equal(scores[i, :k], d["scores"]) and torch.equal(labels[i, :k], d["labels"])
    lib.ymi_plan_destroy(plan2)
