"""Merge-NMS (include/yolort_amd.h YMI_POST_MERGE / YMI_POST_MERGE_KEEP_SINGLE; Python `merge=True`, `merge_redundant=`) on the GPU: merge_gather_kernel through
ymi_postprocess on the case table of tests/_merge_cases.py against its float64 yardstick (exact-operand cases bit for bit, general cases within the derived tolerance),
ops.postprocess_logits, and a yolov5n model: fused and unfused head, the post-process graph on and off, a live flip of the attribute, an exported plan, two runs bit for bit."""
import base64
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _merge_cases as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -3.0
KEYS = ("count", "labels", "scores", "boxes")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


def _gpu_run(dev, case, flags, nms=None, k=None, rescale=None, cap=None):
    """one ymi_postprocess through a fresh plan: pre-filled outputs -> CPU tensors + status"""
    from yolort_amd.engine import Plan, View
    heads, nc, n = case["heads"], case["nc"], case["n"]
    kk = nc + 5
    inputs = []
    for ho in heads:
        cs = (3 * kk + 3) // 4 * 4
        t = torch.zeros(n, ho.shape[2], ho.shape[3], cs, device=dev, dtype=torch.float32)
        t[..., : 3 * kk] = ho.to(dev).permute(0, 2, 3, 1, 4).reshape(n, ho.shape[2], ho.shape[3], 3 * kk)
        inputs.append(t)
    plan = Plan(dev, torch.float16)
    views = [View(t.view(-1), 0, n, t.shape[1], t.shape[2], 3 * kk, t.shape[3]) for t in inputs]
    rs = None if rescale is None else torch.tensor(rescale, dtype=torch.float32, device=dev).reshape(n, 3)
    pb = plan.postprocess(views, case["strides"], case["anchors"], nc, case["thr"], case["nms"] if nms is None else nms, k or case["k"], cap or case["cap"], rescale=rs,
                          flags=flags, classes=case["classes"] if flags & M.POST_CLASS_FILTER else None)
    pb.boxes.fill_(FILL), pb.scores.fill_(FILL), pb.labels.fill_(int(FILL)), pb.status_count.fill_(int(FILL)), pb.slab.fill_(FILL)
    plan.run()
    torch.cuda.synchronize()
    return dict(count=pb.count.cpu(), labels=pb.labels.cpu(), scores=pb.scores.cpu(), boxes=pb.boxes.cpu(), slab=pb.slab.cpu(), status=pb.status.cpu())


def _operands(dev, case, flags, exact):
    best = bool(flags & M.POST_BEST_CLASS)
    oracle = M.oracle_candidates(case["pred"], case["thr"], best, case["classes"] if flags & M.POST_CLASS_FILTER else None)
    out = _gpu_run(dev, case, flags & ~(M.POST_MERGE | M.POST_MERGE_KEEP_SINGLE), nms=1.0, k=max(1, max(len(s) for _, s, _ in oracle)))
    assert out["status"][1] == 0
    cands = M.operand_candidates(out)
    M.assert_operands_match_oracle(cands, oracle, exact)
    return cands


def _check_case(dev, case, extra=0):
    base, exact = case["flags"] | extra, case["exact"]
    agnostic = bool(base & M.POST_AGNOSTIC)
    cands = _operands(dev, case, base, exact)
    outs = {}
    for what, f, kw in (("merge", M.POST_MERGE, {}), ("keep-single", M.POST_MERGE | M.POST_MERGE_KEEP_SINGLE, dict(keep_single=True)), ("plain", 0, dict(merge=False))):
        out = _gpu_run(dev, case, base | f)
        assert out["status"][1] == 0 and int(out["status"][4]) == sum(len(s) for _, s, _ in cands), out["status"]
        M.assert_matches(out, M.merge_reference(cands, case["nms"], case["k"], agnostic, **kw), FILL, exact, f"{case['name']} {what}")
        outs[what] = out
    return outs


# ---- the case table ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.LATTICE_CASES)
def test_merge_lattice_cases(dev, name):
    """exact operands: every merged coordinate equals np.float32(num) / np.float32(den) bit for bit, whatever the summation order; counts, labels, scores exact"""
    case = M.lattice_case(name)
    _check_case(dev, case)
    if name == "shared-box":
        for extra in (M.POST_AGNOSTIC, M.POST_BEST_CLASS, M.POST_BEST_CLASS | M.POST_AGNOSTIC):
            _check_case(dev, case, extra)


def test_merge_eligibility_bounds(dev):
    """n = 0, 1, 2, 2999, 3000 in one batch: the images outside 1 < n < 3000 are bit-identical to the unflagged run"""
    outs = _check_case(dev, M.bounds_case())
    for key in KEYS:
        for img in (0, 1, 4):
            assert torch.equal(outs["merge"][key][img], outs["plain"][key][img]) and torch.equal(outs["keep-single"][key][img], outs["plain"][key][img]), (key, img)
    assert outs["merge"]["count"].tolist()[:3] == [0, 1, 1] and outs["merge"]["count"][4] == 300 and outs["merge"]["count"][3] < 300


@pytest.mark.parametrize("run", M.GENERAL_RUNS, ids=lambda r: "-".join(map(str, r[:6])))
def test_merge_general_cases(dev, run):
    """merged coordinates within (2 m + 3) * 2^-24 * max |coordinate| of the float64 mean of the library's own operands (tied to the oracle's candidates)"""
    _check_case(dev, M.general_case(run))


def test_merge_rescale_and_slab(dev):
    """the rescaled output equals fp32 (merged - pad) / gain of the same input's unrescaled output bit for bit; the slab equals the four arrays, zero past the count;
    a capacity overflow marks every row stale"""
    case = M.lattice_case("contributors")
    n, k = case["n"], case["k"]
    rows = [(0.5 + 0.25 * i, 3.0 * i, 7.0 - i) for i in range(n)]
    rows[1] = (0.0, 5.0, 5.0)
    raw, out = _gpu_run(dev, case, M.POST_MERGE), _gpu_run(dev, case, M.POST_MERGE, rescale=rows)
    assert torch.equal(raw["count"], out["count"]) and torch.equal(raw["scores"], out["scores"]) and torch.equal(raw["labels"], out["labels"])
    for i, (gain, px, py) in enumerate(rows):
        c = int(out["count"][i])
        b = raw["boxes"][i, :c].numpy()
        want = b if gain == 0 else ((b - np.array([px, py, px, py], np.float32)).astype(np.float32) / np.float32(gain)).astype(np.float32)
        np.testing.assert_array_equal(out["boxes"][i, :c].numpy(), want)
        row = out["slab"][i]
        assert torch.equal(row[: 4 * c], out["boxes"][i, :c].reshape(-1)) and torch.equal(row[4 * k: 4 * k + c], out["scores"][i, :c])
        assert torch.equal(row[5 * k: 5 * k + c], out["labels"][i, :c].float()) and row[6 * k] == c
        assert (row[4 * c: 4 * k] == 0).all() and (row[4 * k + c: 5 * k] == 0).all() and (row[5 * k + c: 6 * k] == 0).all()
    over = _gpu_run(dev, case, M.POST_MERGE, cap=n * 64)
    assert int(over["status"][1]) & 1 and (over["slab"][:, 6 * k] == -1.0).all()


def test_merge_leaves_a_truncated_image_alone(dev):
    """the crowded image is cut by the score-prefix selection, never merged, and equals the unflagged run bit for bit, status words included"""
    case = M.truncated_case()
    plain, out = _gpu_run(dev, case, 0), _gpu_run(dev, case, M.POST_MERGE)
    assert torch.equal(plain["status"], out["status"]), (plain["status"], out["status"])
    st = out["status"].tolist()
    assert st[4] == sum(case["counts"]) and 4096 + 6 <= st[0] < st[4], st
    for key in KEYS:
        assert torch.equal(plain[key][0], out[key][0]), key
    ref = M.merge_reference(M.oracle_candidates(case["pred"], case["thr"])[1:], case["nms"], case["k"])
    M.assert_matches({key: out[key][1:] for key in KEYS}, ref, FILL, True, "truncated: the small image")


def test_the_kernel_twice_on_the_same_input_is_bit_identical(dev):
    case = M.general_case(M.GENERAL_RUNS[1])
    a, b = _gpu_run(dev, case, case["flags"] | M.POST_MERGE), _gpu_run(dev, case, case["flags"] | M.POST_MERGE)
    for key in KEYS + ("slab", "status"):
        assert torch.equal(a[key], b[key]), key
    assert int(a["count"].sum()) > 100


def test_ops_postprocess_logits_merge(dev):
    from yolort_amd import ops
    case = M.lattice_case("shared-box")
    heads = [h.to(dev) for h in case["heads"]]
    for agnostic in (False, True):
        cands = M.oracle_candidates(case["pred"], case["thr"])
        counts = {}
        for redundant in (True, False):
            dets = ops.postprocess_logits(heads, case["strides"], case["anchors"], case["nc"], case["thr"], case["nms"], case["k"], agnostic=agnostic, merge=True,
                                          merge_redundant=redundant)
            ref = M.merge_reference(cands, case["nms"], case["k"], agnostic, keep_single=not redundant)
            counts[redundant] = [len(d["scores"]) for d in dets]
            for d, r in zip(dets, ref):
                assert len(d["scores"]) == len(r["scores"]) and d["labels"].cpu().tolist() == r["labels"].tolist()
                for j in range(len(r["scores"])):
                    want = r["boxes"][j].astype(np.float32) if r["num"][j] is None else r["num"][j].astype(np.float32) / np.float32(r["den"][j])
                    np.testing.assert_array_equal(d["boxes"][j].cpu().numpy(), want)
        plain = ops.postprocess_logits(heads, case["strides"], case["anchors"], case["nc"], case["thr"], case["nms"], case["k"], agnostic=agnostic)
        assert [len(d["scores"]) for d in plain] == counts[False] != counts[True]   # merge_redundant=False drops nothing; the default does


# ---- a model ---------------------------------------------------------------------------------------------------------------------------------------------------------
ARCH, S, NMS = "yolov5_darknet_pan_n_r60", 320, 0.45
THRESHOLDS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6)   # the first at which both images have 1 < n < 3000 candidates is used (found on the device from the model's own candidates)


def _model(dev, thr=THRESHOLDS[0], **kw):
    from yolort_amd.models import YOLOv5
    from workloads.synth import synth_weights
    m = YOLOv5(arch=ARCH, size=(S, S), score_thresh=thr, nms_thresh=NMS, **kw)
    m.load_state_dict(synth_weights(m.state_dict(), ARCH, seed=0, head_gain=0.8))
    return m.to(dev).half().eval()


def _images(dev):
    from workloads.synth import synth_images
    return [im.to(dev).half() for im in synth_images(2, S, S, seed=5)]   # the canvas size: the rescale is the identity (gain 1, no padding)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("boxes", "scores", "labels"))


def _pack(dets):
    buf = io.BytesIO()
    torch.save([{k: v.cpu() for k, v in d.items()} for d in dets], buf)
    return base64.b64encode(buf.getvalue()).decode()


_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import test_merge_nms_gpu as T
dev = torch.device("cuda:0")
m = T._model(dev, float(sys.argv[1]), merge=True)
print("DETS " + T._pack(m.predict(T._images(dev))))
"""


def _child(env_extra, thr):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests")), repr(thr)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("DETS ")][-1]
    return [{k: v.to("cuda:0") for k, v in d.items()} for d in torch.load(io.BytesIO(base64.b64decode(line[5:])))]


def _all_candidates(m, imgs):
    """every candidate of the model in rank order: the same model with nms_thresh 1.0 (an IoU is never > 1) and detections_per_img = 3000"""
    pp = m.model.post_process
    keep = (pp.nms_thresh, pp.detections_per_img, pp.merge)
    pp.nms_thresh, pp.detections_per_img, pp.merge = 1.0, M.MERGE_MAX_N, False
    allc = m.predict(imgs)
    pp.nms_thresh, pp.detections_per_img, pp.merge = keep
    return [(d["boxes"].float().cpu().numpy(), d["scores"].float().cpu().numpy(), d["labels"].cpu().numpy()) for d in allc]


@pytest.fixture(scope="module")
def thr(dev):
    imgs = _images(dev)
    for t in THRESHOLDS:
        counts = [len(s) for _, s, _ in _all_candidates(_model(dev, t), imgs)]
        print("score_thresh", t, "candidates", counts)
        if all(1 < c < M.MERGE_MAX_N for c in counts):
            return t
    pytest.fail("no threshold of the list leaves both images inside the merge bound")


def test_model_merge_fused_unfused_graph_flip_and_yardstick(dev, thr):
    """yolov5n, two 320 x 320 images through model.predict with merge=True: within tolerance of the yardstick built on the model's own candidates (the same model with
    nms_thresh 1.0 and detections_per_img 3000 returns every candidate in rank order); the unfused head (a fresh child process, YOLORT_AMD_FUSED_HEAD=0) and the per-kernel
    post-process (YOLORT_AMD_POST_GRAPH=0, another child) return the same bits; merge False -> True -> False on the live model returns the first result bit for bit"""
    m, imgs = _model(dev, thr), _images(dev)
    core = m.model
    assert core.fuse_head_decode and core.post_graph
    d_off = m.predict(imgs)
    core.post_process.merge = True
    d_on = m.predict(imgs)
    core.post_process.merge_redundant = False
    d_single = m.predict(imgs)
    core.post_process.merge, core.post_process.merge_redundant = False, True
    assert _same(m.predict(imgs), d_off), "merge False -> True -> False does not return the first result"
    assert not _same(d_on, d_off) and not _same(d_on, d_single) and not _same(d_single, d_off)
    assert _same(_model(dev, thr, merge=True).predict(imgs), d_on) and _same(_model(dev, thr, merge=True, merge_redundant=False).predict(imgs), d_single)
    cands = _all_candidates(m, imgs)   # the yardstick on the model's own candidates
    print("candidates", [len(s) for _, s, _ in cands], "detections off / on / keep-single", [[len(d["scores"]) for d in ds] for ds in (d_off, d_on, d_single)])
    assert all(1 < len(s) < M.MERGE_MAX_N for _, s, _ in cands)
    for dets, kw in ((d_on, {}), (d_single, dict(keep_single=True)), (d_off, dict(merge=False))):
        ref = M.merge_reference(cands, NMS, 300, False, **kw)
        for d, r in zip(dets, ref):
            assert len(d["scores"]) == len(r["scores"]) and d["labels"].cpu().tolist() == r["labels"].tolist()
            np.testing.assert_array_equal(d["scores"].cpu().numpy(), r["scores"])
            err = np.abs(d["boxes"].cpu().numpy().astype(np.float64) - r["boxes"])
            assert (err <= r["tol"]).all(), float((err - r["tol"]).max())
    M.assert_not_vacuous(M.merge_reference(cands, NMS, 300, False), "yolov5n")
    assert _same(_child({"YOLORT_AMD_FUSED_HEAD": "0"}, thr), d_on), "fused and unfused head disagree"
    assert _same(_child({"YOLORT_AMD_POST_GRAPH": "0"}, thr), d_on), "the post-process graph and the per-kernel launches disagree"


def test_exported_plan_with_merge_replays_to_the_same_detections(dev, tmp_path, thr):
    from yolort_amd import _lib
    from yolort_amd._lib import PlanRegion, TAG_BOXES, TAG_INPUT, TAG_LABELS, TAG_RESCALE, TAG_SCORES, TAG_STATUS_COUNT
    lib = _lib.load(require_gpu=True)
    from workloads.synth import synth_images
    m = _model(dev, thr, merge=True)
    imgs = [synth_images(1, S - 40, S, seed=21)[0].to(dev).half(), synth_images(1, S, S - 64, seed=22)[0].to(dev).half()]   # letterboxed: the exported (canvas) form of the plan
    dets = m.predict(imgs)
    plain = _model(dev, thr).predict(imgs)
    torch.cuda.synchronize()
    assert sum(len(d["scores"]) for d in dets) > 0 and not _same(dets, plain)
    e = next(iter(m.model._entries.values()))
    path = str(tmp_path / "merge.ymiplan")
    info = m.model.export_plan(path, e.x.n, e.x.h, e.x.w, dev)
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
        assert sc[1].item() == 0 and cnt == [len(d["scores"]) for d in dets], (sc[:8].tolist(), cnt)
        for i, d in enumerate(dets):
            k = cnt[i]
            assert torch.equal(boxes[i, :k], d["boxes"]) and torch.equal(scores[i, :k], d["scores"]) and torch.equal(labels[i, :k], d["labels"])
    finally:
        lib.ymi_plan_destroy(plan2)
