"""Shared by tests/test_agnostic_nms.py (CPU: host logic, the simulator) and tests/test_agnostic_nms_gpu.py (the real kernels): inputs and references of the
CLASS-AGNOSTIC NMS (include/yolort_amd.h YMI_POST_AGNOSTIC, ymi_nms; Python `agnostic=True`, ops.nms) and the conditions, computed from the oracle alone, under which a
case says anything.

The reference is the oracle's class-aware NMS with every label equal: O.batched_nms(boxes, scores, zeros_like(labels), thr) -- torchvision.ops.nms on the unshifted
boxes, what ultralytics does with agnostic=True.  Candidates are the oracle's (multi-label: box_head.py:418) or the best-class restatement of
tests/_best_cases.py::best_postprocess (general.py:572-583); the labels are zeroed for the NMS call only, the kept detections carry their own."""
import functools

import numpy as np
import torch

import _post_cases as P

POST_AGNOSTIC, POST_BEST_CLASS, POST_EXACT_FULL = 4, 2, 1   # include/yolort_amd.h (restated so that a missing constant fails a test, not the collection)
NMSB_THREADS = 1024   # threads of the workgroup that walks a segment (postprocess.hip nms_block_kernel: NMSB_WAVES * 64)
NMSB_KCAP = 2048      # kept boxes it holds in LDS; the rest of a segment's kept boxes live in the spill area

# the cases of _post_cases.NMS_CASES whose agnostic kept list differs from the class-aware one (computed from the oracle; asserted by the tests for exactly these names).
# The others have one class, or classes that never share a cell: they are run for what they reach in the kernel (ties, IoU == threshold and 0/0, the spill)
NMS_DIFFER = frozenset(["signed-random", "signed-zeros", "all-negative", "extremes", "far-plus-1e6", "far-minus-1e6", "scaled-1e-3", "own-class"]
                       + [f"segment-{m}" for m in P.SEGMENT_LENGTHS])
SIM_NMS_CASES = ("signed-zeros", "degenerate-half", "radix-257", "segment-65")

# segment length is n itself: around the 64-lane step, and one below / at / above the block size and twice the block size
LENGTHS = (1, 63, 64, 65, 127, 128, 129, NMSB_THREADS - 1, NMSB_THREADS, NMSB_THREADS + 1, 2 * NMSB_THREADS - 1, 2 * NMSB_THREADS, 2 * NMSB_THREADS + 1)
SPILL_SIDE = 50   # grid_boxes(50): 7500 boxes, 2500 kept -- at least 64 more than NMSB_KCAP (asserted from the oracle's count)


def _oracle():
    from oracle import yolov5_oracle as O
    return O


def nms_refs(case):
    """-> (agnostic kept list, class-aware kept list) of the oracle, int64 arrays"""
    O = _oracle()
    b, s, lab = torch.from_numpy(case["boxes"]), torch.from_numpy(case["scores"]), torch.from_numpy(case["labels"])
    return O.batched_nms(b, s, torch.zeros_like(lab), case["thr"]).numpy(), O.batched_nms(b, s, lab, case["thr"]).numpy()


@functools.lru_cache(maxsize=None)
def nms_case_and_refs(name):
    case = P.nms_case(name)
    return (case,) + nms_refs(case)


@functools.lru_cache(maxsize=None)
def length_case(n):
    """n boxes, three to a cell, three random labels, scores rounded to two digits (ties) -> (case, agnostic ref, class-aware ref)"""
    rng = np.random.default_rng(1000 + n)
    boxes = P.cluster_boxes(rng, n)[0]
    case = dict(boxes=np.ascontiguousarray(boxes, np.float32), scores=np.round(rng.random(n), 2).astype(np.float32), labels=rng.integers(0, 3, n).astype(np.int64), thr=0.45)
    return (case,) + nms_refs(case)


def assert_length_case_is_not_vacuous(n, case, ref):
    if n >= 63:
        assert n - len(ref) >= n / 4, f"n={n}: the oracle suppresses only {n - len(ref)}"
        assert len(np.unique(case["scores"])) < n, f"n={n}: no score tie"


@functools.lru_cache(maxsize=None)
def spill_case():
    boxes = P.grid_boxes(SPILL_SIDE)
    n = len(boxes)
    case = dict(boxes=boxes, scores=np.random.default_rng(SPILL_SIDE).random(n).astype(np.float32), labels=np.zeros(n, np.int64), thr=0.45)
    ref, _ = nms_refs(case)
    assert len(ref) >= NMSB_KCAP + 64, f"the oracle keeps {len(ref)}: the spill area is not reached"
    return case, ref


# ---- whole post-process --------------------------------------------------------------------------------------------------------------------------------------------
POST_SHAPES = [(20, 24), (10, 12), (5, 6)]
SIM_SHAPES = [(10, 12), (5, 6), (3, 3)]     # the levels the simulator's post-process tests use (a quarter of the pixels)
POST_NC = (1, 2, 80)
POST_RUNS = (("full", 0.3, 300), ("full", 0.05, 7), ("full", 0.05, 300), ("middle-empty", 0.3, 300), ("all-empty", 0.3, 300))


def post_reference(pred, thr, nms, k, best, agnostic=True):
    """O.postprocess (multi-label) / _best_cases.best_postprocess (best-class) on the oracle's decode, with the labels zeroed for the NMS call only"""
    O = _oracle()
    dets = []
    for p in pred:
        scores = p[:, 5:] * p[:, 4:5]
        cx, cy, w, h = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
        boxes = torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)
        if best:
            conf, j = scores.max(1)
            keep = conf > thr
            b, s, lab = boxes[keep], conf[keep], j[keep]
        else:
            inds, lab = torch.where(scores > thr)
            b, s = boxes[inds], scores[inds, lab]
        kept = O.batched_nms(b, s, torch.zeros_like(lab) if agnostic else lab, nms)[:k]
        dets.append({"scores": s[kept], "labels": lab[kept], "boxes": b[kept]})
    return dets


@functools.lru_cache(maxsize=None)
def post_inputs(nc, variant, sim=False):
    O = _oracle()
    strides, anchors = O.anchors_for(3)
    heads = P.post_heads(nc, SIM_SHAPES if sim else POST_SHAPES, n=3, empty=P.POST_EMPTY[variant])
    return heads, list(strides), [list(map(float, a)) for a in anchors], O.decode(heads, strides, anchors)


@functools.lru_cache(maxsize=None)
def post_full_ref(nc, variant, thr, best, agnostic=True, sim=False):
    """the un-truncated survivors (the top-k cut is a slice of them); computed once, left unchanged"""
    return post_reference(post_inputs(nc, variant, sim)[3], thr, 0.45, 1 << 30, best, agnostic)


def cut(full, k):
    return [{key: v[:k] for key, v in r.items()} for r in full]


def differs(a, b):
    """per image: do two detection lists differ (count, labels or scores)"""
    return [len(x["scores"]) != len(y["scores"]) or not torch.equal(x["labels"], y["labels"]) or not torch.equal(x["scores"], y["scores"]) for x, y in zip(a, b)]


def assert_post_case_is_not_vacuous(nc, variant, thr, k, best, sim=False):
    """from the oracle alone: images listed as empty have no survivor, the others have; with more than one class every `full` run with k = 300 has an image whose agnostic
    top-k differs from the class-aware top-k; with one class the two agree everywhere -> (agnostic survivors per image, images that differ)"""
    full = post_full_ref(nc, variant, thr, best, True, sim)
    aware = post_full_ref(nc, variant, thr, best, False, sim)
    survivors = [len(r["scores"]) for r in full]
    for i, c in enumerate(survivors):
        assert (c == 0) == (i in P.POST_EMPTY[variant]), (variant, survivors)
    d = differs(cut(full, k), cut(aware, k))
    if nc == 1:
        assert not any(d)
    elif variant == "full" and k == 300:
        assert any(d), f"nc={nc} thr={thr} best={best}: the agnostic and the class-aware top-{k} agree in every image"
    return survivors, d


@functools.lru_cache(maxsize=None)
def crowded_inputs(aw):
    """the crowded image of tests/test_ops_gpu.py::test_postprocess_score_prefix_vs_oracle (seed 31, 48 x 48, nc 4)"""
    O = _oracle()
    g = torch.Generator().manual_seed(31)
    nc = 4
    heads = [torch.randn(2, 3, 48, 48, nc + 5, generator=g)]
    heads[0][..., :4] *= 0.05
    heads[0][1] -= 6.0
    heads[0][0, ..., 4:] += 3.0
    strides, anchors = [8], [[aw, aw, 1.1 * aw, 0.9 * aw, 0.9 * aw, 1.1 * aw]]
    return heads, strides, anchors, O.decode(heads, strides, anchors)


@functools.lru_cache(maxsize=None)
def global_inputs(n):
    """the global-sort path (cand_cap / n < 64): n images, one 2 x 2 level at stride 8, nc 3, at most 36 candidates an image"""
    O = _oracle()
    g = torch.Generator().manual_seed(64)
    heads = [torch.randn(n, 3, 2, 2, 8, generator=g) + 1.0]
    strides, anchors = [8], [list(map(float, O.ANCHORS_P5[2]))]
    return heads, strides, anchors, O.decode(heads, strides, anchors)


GLOBAL = dict(nc=3, thr=0.3, k=10, per_image_cap=48)


# ---- the real kernels through the plan, under the host protocol of yolort_amd/ops.py (the mode flags stay set in every redo) ----
def gpu_post(dev, heads, strides, anchors, nc, thr, k, cap, flags, fill=-3.0):
    from yolort_amd.engine import Plan, View
    n, kk = heads[0].shape[0], nc + 5
    inputs = []
    for ho in heads:
        cs = (3 * kk + 3) // 4 * 4
        t = torch.zeros(n, ho.shape[2], ho.shape[3], cs, device=dev, dtype=torch.float32)
        t[..., : 3 * kk] = ho.to(dev).permute(0, 2, 3, 1, 4).reshape(n, ho.shape[2], ho.shape[3], 3 * kk)
        inputs.append(t)
    passes = []
    while True:
        plan = Plan(dev, torch.float16)
        views = [View(t.view(-1), 0, n, t.shape[1], t.shape[2], 3 * kk, t.shape[3]) for t in inputs]
        pb = plan.postprocess(views, strides, anchors, nc, thr, 0.45, k, cap, flags=flags)
        pb.boxes.fill_(fill), pb.scores.fill_(fill), pb.labels.fill_(int(fill)), pb.status_count.fill_(int(fill))
        plan.run()
        st = pb.status.cpu().tolist()
        passes.append(st)
        assert len(passes) <= 6, passes
        if st[1] == 0:
            return dict(count=pb.count.cpu(), labels=pb.labels.cpu(), scores=pb.scores.cpu(), boxes=pb.boxes.cpu(), passes=passes, cap=cap)
        if not st[1] & 1:
            flags |= POST_EXACT_FULL
            continue
        need = max(st[0], st[3] * n)
        cap = max(int(need * 1.25) + 1024, 2 * cap)
        cap = n * (1 << ((cap + n - 1) // n - 1).bit_length())


def gpu_runs():
    """(key, heads, strides, anchors, nc, thr, k, cap, flags) of the runs the bit-identity test repeats in a child process with YOLORT_AMD_NMS_BLOCK=0:
    the class counts 2 and 80 of the whole post-process in both modes, and the global-sort path"""
    for nc in (2, 80):
        for best in (False, True):
            for variant, thr, k in POST_RUNS:
                heads, strides, anchors, _ = post_inputs(nc, variant)
                yield (f"post-nc{nc}-{'best' if best else 'multi'}-{variant}-{thr}-{k}", heads, strides, anchors, nc, thr, k, 3 * 8192, POST_AGNOSTIC | (POST_BEST_CLASS if best else 0))
    for best in (False, True):
        heads, strides, anchors, _ = global_inputs(64)
        yield (f"global-{'best' if best else 'multi'}", heads, strides, anchors, GLOBAL["nc"], GLOBAL["thr"], GLOBAL["k"], 64 * GLOBAL["per_image_cap"],
               POST_AGNOSTIC | (POST_BEST_CLASS if best else 0))
