"""Class-agnostic NMS (include/yolort_amd.h YMI_POST_AGNOSTIC and ymi_nms; Python `agnostic=True`, ops.nms) on the GPU: the workgroup-per-segment kernel
(postprocess.hip nms_block_kernel) stand-alone and inside the whole post-process on both sort paths, against the oracle with every label equal
(tests/_agnostic_cases.py), against its one-wave counterpart bit for bit (YOLORT_AMD_NMS_BLOCK=0 in a fresh child process), and a whole model: fused = unfused =
ops.postprocess_logits, the flag flipped on a live model, an exported plan, the fp32 parity mode."""
import base64
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _agnostic_cases as A
import _head_cases as H
import _post_cases as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -3.0
KEYS = ("count", "labels", "scores", "boxes")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


def _pass_words(passes):
    """what is reproducible of the status words of a run's passes: the overflow / prefix bits of every pass and all words of the last one.  (The record count of a pass
    that OVERFLOWED its capacity is not: which records made it into the regions depends on the order of the producers' atomic appends.)"""
    return [p[1] for p in passes], passes[-1]


def _nms(dev, case):
    from yolort_amd.ops import nms
    got = nms(torch.from_numpy(case["boxes"]).to(dev), torch.from_numpy(case["scores"]).to(dev), case["thr"])
    assert got.dtype == torch.int64
    return got.cpu().numpy()


# ---- stand-alone ops.nms / ymi_nms ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.NMS_CASES)
def test_nms_adversarial_vs_oracle(dev, name):
    """every case of _post_cases.NMS_CASES with the labels ignored: kept indices equal the oracle's with every label equal, element for element.  For the names of
    A.NMS_DIFFER -- and for no other -- that list differs from the class-aware one: a kernel that still honoured labels cannot pass.  The others are run for what they
    reach: ties at equal scores (radix-*), IoU == threshold and 0/0 (degenerate-*), signed / extreme scores."""
    case, ref, aware = A.nms_case_and_refs(name)
    print(f"{name}: n={len(case['scores'])} agnostic keeps {len(ref)}, class-aware keeps {len(aware)}")
    assert (not np.array_equal(ref, aware)) == (name in A.NMS_DIFFER)
    np.testing.assert_array_equal(_nms(dev, case), ref)


@pytest.mark.parametrize("n", A.LENGTHS)
def test_nms_segment_lengths_vs_oracle(dev, n):
    """the segment is the whole input: lengths around the 64-candidate step, the block size and twice the block size; at least a quarter suppressed, score ties"""
    case, ref, aware = A.length_case(n)
    A.assert_length_case_is_not_vacuous(n, case, ref)
    np.testing.assert_array_equal(_nms(dev, case), ref)


def test_nms_spill_vs_oracle(dev):
    """the oracle keeps at least 64 boxes more than the block holds in LDS: the rest is written to the spill area by one wave and read back by all of them -- only
    hardware says whether they see it"""
    case, ref = A.spill_case()
    np.testing.assert_array_equal(_nms(dev, case), ref)


def test_nms_edge_calls(dev):
    from yolort_amd._lib import YmiError
    from yolort_amd.ops import batched_nms, nms
    got = nms(torch.zeros(0, 4, device=dev), torch.zeros(0, device=dev), 0.45)
    assert got.dtype == torch.int64 and got.numel() == 0
    n = 1 << 20
    with pytest.raises(YmiError, match=f"ymi_nms.*out of range.*{n - 1}"):
        nms(torch.zeros(n, 4, device=dev), torch.zeros(n, device=dev), 0.45)
    with pytest.raises(YmiError):
        nms(torch.zeros(4, 4), torch.zeros(4), 0.45)
    # the one-wave kernel (batched_nms with zero labels) and the block kernel agree at the op level
    case, ref, _ = A.nms_case_and_refs("signed-random")
    b, s = torch.from_numpy(case["boxes"]).to(dev), torch.from_numpy(case["scores"]).to(dev)
    one_wave = batched_nms(b, s, torch.zeros(len(s), dtype=torch.int64, device=dev), case["thr"])
    assert torch.equal(nms(b, s, case["thr"]), one_wave) and len(one_wave) == len(ref)


# ---- whole post-process with the flag ------------------------------------------------------------------------------------------------------------------------------
_RESULTS = {}


def _run(dev, key, *args):
    """one run of A.gpu_runs (or of a test's own), cached for the bit-identity test and left unchanged"""
    if key not in _RESULTS:
        _RESULTS[key] = A.gpu_post(dev, *args, fill=FILL)
    return _RESULTS[key]


@pytest.mark.parametrize("best", [False, True])
@pytest.mark.parametrize("nc", A.POST_NC)
def test_postprocess_agnostic_vs_oracle(dev, nc, best):
    """three images on levels (20, 24), (10, 12), (5, 6), every run of A.POST_RUNS with YMI_POST_AGNOSTIC, multi-label and best-class candidates: counts, labels, order
    exact; scores rtol 2e-6 / atol 1e-7, boxes rtol 1e-5 / atol 1e-4; slots past the count keep their fill.  nc = 1: bit-identical to the flag-less run.  nc = 80, 0.3,
    multi-label: the agnostic survivors stay below k, the score prefix falls short on the first pass and the exact full pass follows.  nc = 80, 0.05, multi-label:
    about 25 000 candidates an image, the multi-run sort."""
    flags = A.POST_AGNOSTIC | (A.POST_BEST_CLASS if best else 0)
    for variant, thr, k in A.POST_RUNS:
        survivors, d = A.assert_post_case_is_not_vacuous(nc, variant, thr, k, best)
        heads, strides, anchors, _ = A.post_inputs(nc, variant)
        got = _run(dev, f"post-nc{nc}-{'best' if best else 'multi'}-{variant}-{thr}-{k}", heads, strides, anchors, nc, thr, k, 3 * 8192, flags)
        print(f"nc={nc} best={best} {variant} thr={thr} k={k}: survivors {survivors} differ {d} passes {[p[:5] for p in got['passes']]} cap {got['cap']}")
        H.assert_equals_oracle(got, A.cut(A.post_full_ref(nc, variant, thr, best), k), FILL)
        if nc == 1:
            plain = A.gpu_post(dev, heads, strides, anchors, nc, thr, k, 3 * 8192, flags & ~A.POST_AGNOSTIC, fill=FILL)
            for key in KEYS:
                assert torch.equal(plain[key], got[key]), (variant, thr, k, key)
            assert _pass_words(plain["passes"]) == _pass_words(got["passes"])
        if nc == 80 and not best and variant == "full" and thr == 0.3:
            assert max(survivors) < k and got["passes"][0][1] & 2 and len(got["passes"]) == 2, got["passes"]


@pytest.mark.parametrize("best", [False, True])
@pytest.mark.parametrize("aw,expect_short", [(30.0, False), (400.0, True)])
def test_postprocess_agnostic_score_prefix_vs_oracle(dev, aw, expect_short, best):
    """the crowded image of test_postprocess_score_prefix_vs_oracle under the flag.  aw = 30: 855 agnostic survivors, 300 of them inside the score prefix: one pass.
    aw = 400: 8 survivors: YMI_STATUS_PREFIX_SHORT, then the exact full pass."""
    heads, strides, anchors, pred = A.crowded_inputs(aw)
    ref = A.post_reference(pred, 0.3, 0.45, 300, best)
    got = A.gpu_post(dev, heads, strides, anchors, 4, 0.3, 300, 2 * 32768, A.POST_AGNOSTIC | (A.POST_BEST_CLASS if best else 0), fill=FILL)
    print("passes", [p[:5] for p in got["passes"]])
    H.assert_equals_oracle(got, ref, FILL)
    first = got["passes"][0]
    assert bool(first[1] & 2) == expect_short and not first[1] & 1 and len(got["passes"]) == (2 if expect_short else 1)
    if not best:
        assert first[0] < 3 * 48 * 48 * 4, "the first image should have been cut to a prefix"


@pytest.mark.parametrize("best", [False, True])
def test_postprocess_agnostic_global_sort_path_vs_oracle(dev, best):
    """cand_cap / n < 64: the global radix sort, label 0 and no label pass, one segment per image; 64 images of which 64 (63 in best-class mode) differ from their
    class-aware result; one pass, no capacity growth"""
    g = A.GLOBAL
    heads, strides, anchors, pred = A.global_inputs(64)
    ref = A.post_reference(pred, g["thr"], 0.45, g["k"], best)
    d = A.differs(ref, A.post_reference(pred, g["thr"], 0.45, g["k"], best, agnostic=False))
    assert sum(d) == (63 if best else 64)
    got = _run(dev, f"global-{'best' if best else 'multi'}", heads, strides, anchors, g["nc"], g["thr"], g["k"], 64 * g["per_image_cap"], A.POST_AGNOSTIC | (A.POST_BEST_CLASS if best else 0))
    assert len(got["passes"]) == 1 and got["passes"][0][1] == 0 and got["passes"][0][2] == 64 and got["cap"] == 64 * g["per_image_cap"], got["passes"]
    H.assert_equals_oracle(got, ref, FILL)


_CHILD = r"""
import base64, io, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import _agnostic_cases as A
dev = torch.device("cuda:0")
for key, *args in A.gpu_runs():
    got = A.gpu_post(dev, *args, fill=%r)
    buf = io.BytesIO()
    np.savez_compressed(buf, passes=np.array(got["passes"]), **{k: got[k].numpy() for k in ("count", "labels", "scores", "boxes")})
    print("DET", key, base64.b64encode(buf.getvalue()).decode(), flush=True)
print("DONE")
"""


def test_block_kernel_is_bit_identical_to_the_one_wave_counterpart(dev):
    """YOLORT_AMD_NMS_BLOCK=0 (read once per process: a fresh child) sends the agnostic segments through nms_segments_kernel, one wave per image.  The runs of
    A.gpu_runs -- the whole post-process at nc = 2 and 80 in both modes, and the global-sort path -- return the same arrays and counts as this process's, and the same status words (see _pass_words)."""
    env = dict(os.environ, YOLORT_AMD_NMS_BLOCK="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), FILL)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("DONE"), (r.returncode, r.stderr[-3000:])
    seen = set()
    for line in r.stdout.splitlines():
        if not line.startswith("DET "):
            continue
        _, key, blob = line.split(" ", 2)
        z = np.load(io.BytesIO(base64.b64decode(blob)))
        args = next(a for a in A.gpu_runs() if a[0] == key)
        mine = _run(dev, *args)
        for k in KEYS:
            assert torch.equal(torch.from_numpy(z[k]), mine[k]), f"{key}: the one-wave kernel differs from the block kernel in {k}"
        assert _pass_words(z["passes"].tolist()) == _pass_words(mine["passes"]), key
        seen.add(key)
    assert seen == {a[0] for a in A.gpu_runs()}, seen


# ---- whole model ---------------------------------------------------------------------------------------------------------------------------------------------------
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


def _logit_heads(e):
    heads = []
    for v in e.logits:
        t = v.as_tensor()
        heads.append(t.reshape(t.shape[0], t.shape[1], t.shape[2], 3, NC + 5).permute(0, 3, 1, 2, 4).contiguous())
    return heads


@pytest.mark.parametrize("multi_label", [True, False])
def test_whole_model_fused_unfused_and_postprocess_logits_agree(dev, multi_label):
    """yolov5n with seeded weights on two 3 x 96 x 128 images, agnostic=True: the fused head equals the stored-logits form bit for bit, both equal
    ops.postprocess_logits(head outputs, agnostic=True), and the class-aware result differs"""
    from yolort_amd.ops import postprocess_logits
    m, x = _model(dev, multi_label=multi_label, agnostic=True), _batch(dev)
    assert m.model.post_process.agnostic is True and m.model.fuse_head_decode
    fused = m.model(x)
    m.model.fuse_head_decode = False
    unfused = m.model(x)
    e = next(iter(m.model._entries.values()))
    assert e.logits is not None
    assert _same(fused, unfused), "fused / unfused head disagree under agnostic=True"
    ag, pp = m.model.anchor_generator, m.model.post_process
    args = (_logit_heads(e), [float(s) for s in ag.strides], ag.anchor_grids, NC, float(pp.score_thresh), float(pp.nms_thresh), int(pp.detections_per_img))
    want = postprocess_logits(*args, multi_label=multi_label, agnostic=True)
    assert _same(unfused, want), "model / postprocess_logits disagree under agnostic=True"
    aware = postprocess_logits(*args, multi_label=multi_label)
    n_det = [len(d["scores"]) for d in fused]
    print("detections", n_det, "class-aware", [len(d["scores"]) for d in aware])
    assert sum(n_det) > 10 and not _same(aware, want)


def test_toggling_agnostic_on_a_live_model_takes_effect_on_the_next_batch(dev):
    """no stale plan: the detections change with `post_process.agnostic` and change back, with the fused and with the unfused head"""
    m, x = _model(dev), _batch(dev)
    for fused in (True, False):
        m.model.fuse_head_decode = fused
        m.model.post_process.agnostic = False
        aware = m.model(x)
        m.model.post_process.agnostic = True
        agn = m.model(x)
        m.model.post_process.agnostic = False
        again = m.model(x)
        assert _same(aware, again) and not _same(aware, agn), fused
        ref = _model(dev, agnostic=True)
        ref.model.fuse_head_decode = fused
        assert _same(agn, ref.model(x)), fused


def test_fp32_parity_mode_agrees_on_labels_and_counts(dev):
    from yolort_amd.ops import postprocess_logits
    x = _batch(dev)
    m32 = _model(dev, torch.float32, agnostic=True)
    m32.set_compute_dtype(torch.float32)
    d32 = m32.model(x.float())
    e = next(iter(m32.model._entries.values()))
    assert e.logits is not None, "the parity mode keeps the fp32 logits"
    ag, pp = m32.model.anchor_generator, m32.model.post_process
    want = postprocess_logits(_logit_heads(e), [float(s) for s in ag.strides], ag.anchor_grids, NC, float(pp.score_thresh), float(pp.nms_thresh), int(pp.detections_per_img), agnostic=True)
    assert sum(len(d["scores"]) for d in d32) > 10
    for d, r in zip(d32, want):
        assert len(d["scores"]) == len(r["scores"]) and torch.equal(d["labels"], r["labels"])


def test_exported_plan_with_the_flag_replays_to_the_same_detections(dev, tmp_path):
    """the descriptor travels with the plan: an exported agnostic plan, replayed through the C ABI alone, returns the model's detections bit for bit"""
    import ctypes as C
    from yolort_amd import _lib
    from yolort_amd._lib import PlanRegion, TAG_BOXES, TAG_INPUT, TAG_LABELS, TAG_RESCALE, TAG_SCORES, TAG_STATUS_COUNT
    from workloads.synth import synth_images
    lib = _lib.load(require_gpu=True)
    S = 160
    m = _model(dev, agnostic=True, size=(S, S))
    imgs = [synth_images(1, S - 40, S, seed=21)[0].to(dev).half(), synth_images(1, S, S - 64, seed=22)[0].to(dev).half()]
    dets = m.predict(imgs)
    torch.cuda.synchronize()
    m.model.post_process.agnostic = False
    aware = m.predict(imgs)
    m.model.post_process.agnostic = True
    assert sum(len(d["scores"]) for d in dets) > 0 and not _same(dets, aware)
    assert _same(dets, m.predict(imgs))
    e = next(iter(m.model._entries.values()))
    path = str(tmp_path / "agnostic.ymiplan")
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
