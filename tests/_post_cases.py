"""Shared by tests/test_ops_gpu.py (the real kernels) and tests/test_hipsim_kernels.py (the same sources on the CPU simulator): seeded ADVERSARIAL inputs of the
detection post-process (yolort_amd/csrc/postprocess.hip) and the conditions, computed from the oracle's result alone, under which a case says anything.

Stand-alone NMS: signed / zero / infinite / subnormal scores (the sort key), segments that keep more than NMS_KCAP = 384 boxes (the HBM spill), degenerate boxes
and IoU equal to the threshold, far coordinates, segment lengths around the 64-lane ballot step, record counts around the radix pass boundaries.
Whole post-process: head logits for any class count, with a pixel that passes more records than the decode's 512-record wave buffer holds."""
import numpy as np
import torch

NMS_KCAP = 384   # kept boxes a wave holds in LDS (postprocess.hip); the rest of a segment's kept boxes live in the spill area


def rand_boxes(rng, n, span=200.0):
    xy = rng.random((n, 2), dtype=np.float32) * np.float32(span)
    wh = rng.random((n, 2), dtype=np.float32) * 60 + 2
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def grid_boxes(side=30):
    """side x side disjoint 8 px boxes at pitch 10, each present three times: exact, jittered by +-1 px, exact again.  Per class the greedy NMS keeps one box
    per cell the class occurs in (jitter by one pixel: IoU >= 0.62) and nothing suppresses across cells."""
    rng = np.random.default_rng(side)
    gy, gx = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    x1, y1 = (gx.reshape(-1) * 10).astype(np.float32), (gy.reshape(-1) * 10).astype(np.float32)
    exact = np.stack([x1, y1, x1 + 8, y1 + 8], 1)
    jit = rng.choice(np.array([-1.0, 1.0], np.float32), (side * side, 2))
    jittered = exact + np.concatenate([jit, jit], 1)
    return np.concatenate([exact, jittered, exact], 0).astype(np.float32)


def cluster_boxes(rng, n, per=3):
    """n boxes in shuffled order, `per` to a cell of a pitch-10 lattice, each shifted by -1 / 0 / +1 px per axis: heavy suppression inside a cell, none across cells"""
    cell = rng.permutation(n) // per
    side = int(np.ceil(np.sqrt(cell.max() + 1)))
    x1, y1 = (cell % side * 10).astype(np.float32), (cell // side * 10).astype(np.float32)
    sh = rng.integers(-1, 2, (n, 2)).astype(np.float32)
    return np.stack([x1 + sh[:, 0], y1 + sh[:, 1], x1 + 8 + sh[:, 0], y1 + 8 + sh[:, 1]], 1).astype(np.float32), cell


def lattice_boxes(rng, n, positions=3):
    """corners on a 4 px lattice, extents from {-4, 0, 4, 8, 12}: zero areas (IoU = 0/0), negative extents, exact duplicates, IoU of exactly 0, 1/3, 1/2 and 1.
    Only the 9 / 25 of the boxes with two positive extents can be suppressed at all, so the lattice is tiny (positions x positions corners): on 8 x 8 the oracle
    suppresses 98 (IoU > 1/3) and 42 (IoU > 1/2) of 600, on 3 x 3 in one class about 200 and 180"""
    xy = rng.integers(0, positions, (n, 2)).astype(np.float32) * 4
    ext = rng.choice(np.array([-4, 0, 4, 8, 12], np.float32), (n, 2))
    return np.concatenate([xy, xy + ext], 1).astype(np.float32)


F32_MAX, F32_MIN_NORMAL = np.finfo(np.float32).max, np.finfo(np.float32).tiny
F32_SUB_MAX, F32_SUB_MIN = np.float32(F32_MIN_NORMAL) - np.float32(1e-45), np.float32(1e-45)   # largest / smallest subnormal
EXTREMES = np.array([np.inf, -np.inf, F32_MAX, -F32_MAX, F32_MIN_NORMAL, -F32_MIN_NORMAL, F32_SUB_MAX, -F32_SUB_MAX, F32_SUB_MIN, -F32_SUB_MIN, 0.0, -0.0, 1.0, -1.0], np.float32)

DEGENERATE_THRESHOLDS = {"0": 0.0, "third": 1.0 / 3.0, "half": 0.5, "1": 1.0}
SEGMENT_LENGTHS = (63, 64, 65, 127, 128, 129)
RADIX_COUNTS = (2, 16, 17, 255, 256, 257, 4095, 4096, 4097)

NMS_CASES = (["signed-grid", "signed-random", "signed-zeros", "all-negative", "extremes", "spill", "spill-one-class"]
             + ["degenerate-" + k for k in DEGENERATE_THRESHOLDS] + ["far-plus-1e6", "far-minus-1e6", "scaled-1e-3"]
             + [f"segment-{m}" for m in SEGMENT_LENGTHS] + [f"radix-{m}" for m in RADIX_COUNTS] + ["own-class"])
SIGNED_CASES = ("signed-grid", "signed-random", "signed-zeros", "all-negative", "extremes")   # the cases the non-negative-only sort key got wrong


def nms_case(name):
    """-> dict(boxes (n,4) f32, scores (n,) f32, labels (n,) i64, thr, quarter, per_class): `quarter` / `per_class` say which halves of the vacuity condition apply"""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    rng = np.random.default_rng(seed)
    thr, quarter, per_class = 0.45, True, True
    if name in ("signed-grid", "spill", "spill-one-class"):
        boxes = grid_boxes(30)
        n = len(boxes)
        labels = np.arange(n) % 2 if name != "spill-one-class" else np.zeros(n)
        scores = np.random.default_rng(0).standard_normal(n) if name == "signed-grid" else rng.random(n)
    elif name == "signed-random":
        n = 5000
        boxes, scores, labels = rand_boxes(rng, n), rng.standard_normal(n), rng.integers(0, 5, n)
    elif name == "signed-zeros":
        n = 600
        boxes, labels = cluster_boxes(rng, n, per=4)[0], rng.integers(0, 2, n)
        scores = rng.choice(np.array([-0.0, 0.0, 0.5, -1.0], np.float32), n)
    elif name == "all-negative":
        n = 3000
        boxes, labels = rand_boxes(rng, n), rng.integers(0, 4, n)
        scores = -np.round(rng.random(n), 2)
    elif name == "extremes":
        n = 900
        boxes, labels = cluster_boxes(rng, n, per=4)[0], rng.integers(0, 3, n)
        scores = np.where(rng.random(n) < 0.7, rng.choice(EXTREMES, n), rng.standard_normal(n).astype(np.float32) * np.float32(1e-38))
    elif name.startswith("degenerate-"):
        n = 600
        thr = DEGENERATE_THRESHOLDS[name.split("-", 1)[1]]
        quarter = thr not in (0.0, 1.0)    # IoU > 1 never holds; at 0 the input is run for the 0/0 and IoU == 0 comparisons
        boxes, labels = lattice_boxes(rng, n), np.zeros(n)
        scores = np.round(rng.random(n), 1)
    elif name in ("far-plus-1e6", "far-minus-1e6", "scaled-1e-3"):
        n = 1500
        boxes, labels, scores = rand_boxes(rng, n), rng.integers(0, 3, n), np.round(rng.random(n), 2)
        boxes = {"far-plus-1e6": boxes + np.float32(1e6), "far-minus-1e6": boxes - np.float32(1e6), "scaled-1e-3": boxes * np.float32(1e-3)}[name]
    elif name.startswith("segment-"):
        m, other = int(name.split("-")[1]), 150
        n = m + other
        labels = rng.permutation(np.concatenate([np.zeros(m), np.ones(other)]))
        boxes, scores = cluster_boxes(rng, n)[0], np.round(rng.random(n), 2)
    elif name.startswith("radix-"):
        n = int(name.split("-")[1])
        ncls = 1 if n <= 17 else (3 if n <= 257 else 8)
        boxes, cell = cluster_boxes(rng, n)
        labels, scores = cell % ncls, np.full(n, 0.25)    # a cell's boxes share a class
        per_class = n > 2   # two candidates cannot both lose a quarter and keep two: n = 2 is a pair of which the SECOND (equal score, later index) must go
        if n == 2:
            boxes[1] = boxes[0]
    elif name == "own-class":
        n = 4096
        boxes, labels, scores = rand_boxes(rng, n), rng.permutation(n), np.round(rng.standard_normal(n), 1)
        quarter = per_class = False
    else:
        raise KeyError(name)
    return dict(boxes=np.ascontiguousarray(boxes, np.float32), scores=np.ascontiguousarray(scores, np.float32), labels=np.ascontiguousarray(labels, np.int64),
                thr=float(thr), quarter=quarter, per_class=per_class)


def iou_f32(a, b):
    """the oracle's formula (oracle/nms_ref.c) in fp32, a: (n, 4) against b: (m, 4) -> (n, m)"""
    a, b = a.astype(np.float32)[:, None, :], b.astype(np.float32)[None, :, :]
    w = np.maximum(np.float32(0), np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]))
    h = np.maximum(np.float32(0), np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]))
    inter = w * h
    area_a, area_b = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]), (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area_a + area_b - inter)


def assert_nms_case_is_not_vacuous(name, case, ref):
    """from the ORACLE's kept list alone: it suppresses at least a quarter of the candidates and keeps more than one per class; plus what the case is there to reach"""
    n, labels = len(case["scores"]), case["labels"]
    kept_per_class = np.bincount(labels[ref], minlength=int(labels.max()) + 1)[np.unique(labels)]
    if case["quarter"]:
        assert n - len(ref) >= n / 4, f"{name}: the oracle suppresses only {n - len(ref)} of {n}"
    if case["per_class"]:
        assert kept_per_class.min() > 1, f"{name}: a class keeps {kept_per_class.min()}"
    if name in ("signed-grid", "spill"):
        assert kept_per_class.max() > NMS_KCAP, f"{name}: no class keeps more than {NMS_KCAP} ({kept_per_class.max()})"
    if name == "spill-one-class":
        assert kept_per_class.max() > 2 * NMS_KCAP, f"{name}: {kept_per_class.max()} kept"
    if name in SIGNED_CASES:
        assert (np.signbit(case["scores"])).any() and not np.isnan(case["scores"]).any()
    if name.startswith("degenerate-"):
        thr = np.float32(case["thr"])
        hit = False
        for c in np.unique(labels):
            b = case["boxes"][labels == c]
            iou = iou_f32(b, b)
            hit |= bool((iou[np.triu_indices(len(b), 1)] == thr).any())
        assert hit, f"{name}: no same-class pair has IoU == {thr}"
        area = (case["boxes"][:, 2] - case["boxes"][:, 0]) * (case["boxes"][:, 3] - case["boxes"][:, 1])
        assert (area == 0).any() and (case["boxes"][:, 2] < case["boxes"][:, 0]).any()
    if name == "own-class":
        assert len(ref) == n
    return kept_per_class


# ---- whole post-process ------------------------------------------------------------------------------------------------------------------------------------------
POST_CLASS_COUNTS = (1, 2, 27, 28, 80, 81, 91, 124, 166, 200, 601)
DEC_BUF = 512    # records the decode kernel buffers per wave (postprocess.hip)


def post_heads(nc, shapes, n=3, seed=11, empty=()):
    """reference-layout head outputs [(n, 3, h, w, nc + 5)], drawn as tests/test_ops_gpu.py draws them for nc = 80 (randn * 2 - 1).  Above 27 classes the objectness of a random
    share of the anchors is lowered so that the candidate count -- the oracle's NMS is quadratic in it -- stays near that of 27 classes.  From 166 classes on (3 * (nc + 5) >
    DEC_BUF channels per pixel) one pixel of the first image and the last pixel of the last image pass EVERY (anchor, class) pair: 498 records at nc = 166 (the most
    166 classes can give; the buffer is flushed before each such pixel), more than DEC_BUF from nc = 171 on (flushed in the middle of the pixel).  Images listed
    in `empty` pass nothing."""
    g = torch.Generator().manual_seed(seed + nc)
    heads = [torch.randn(n, 3, h, w, nc + 5, generator=g) * 2.0 - 1.0 for h, w in shapes]
    for ho in heads:
        if nc > 27:
            off = torch.rand(ho.shape[:4], generator=g) > 27.0 / nc
            ho[..., 4] -= 8.0 * off
        if nc >= 166:
            for img, y, x in ((0, min(3, ho.shape[2] - 1), min(5, ho.shape[3] - 1)), (n - 1, ho.shape[2] - 1, ho.shape[3] - 1)):
                ho[img, :, y, x, 4] = 6.0
                ho[img, :, y, x, 5:] = 5.0 + torch.randn(3, nc, generator=g).round() * 0.25   # rounded: exact score ties inside the pixel
        for img in empty:
            ho[img, ..., 4] = -12.0
    return heads


def oracle_candidates_per_anchor(pred, thr):
    """(n, anchors) number of classes of each anchor whose score passes, from the oracle's decode"""
    return ((pred[..., 5:] * pred[..., 4:5]) > thr).sum(-1)


def hottest_pixel_records(pred, shapes, thr):
    """largest number of (anchor, class) pairs one feature-map pixel passes (a pixel's three anchors are h * w apart inside its level)"""
    cnt = oracle_candidates_per_anchor(pred, thr)
    best, off = 0, 0
    for h, w in shapes:
        best = max(best, int(cnt[:, off: off + 3 * h * w].view(-1, 3, h * w).sum(1).max()))
        off += 3 * h * w
    return best


def post_runs(nc, total_anchors, lean=False):
    """(variant, score_thresh, detections_per_img, truncates) of one class count: the two settings tests/test_ops_gpu.py::test_postprocess_vs_oracle has always used,
    top-k cuts at 1 / 7 / 300 with MORE survivors than that in every image (`truncates`: asserted from the oracle; 300 only where anchors x classes can leave that many),
    a batch whose MIDDLE image has no candidate and a batch without any.  `lean` (the CPU simulator, ~15 s a run): one truncating run and the middle-empty batch
    per class count, the whole list at nc = 2 only"""
    if lean and nc != 2:
        return [("full", 0.05, 7, True), ("middle-empty", 0.3, 300, False)]
    runs = [("full", 0.3, 300, False), ("full", 0.05, 50, True), ("full", 0.05, 1, True), ("full", 0.05, 7, True)]
    if nc >= 2 or total_anchors >= 1000:
        runs.append(("full", 0.05, 300, True))
    return runs + [("middle-empty", 0.3, 300, False), ("all-empty", 0.3, 300, False)]


POST_EMPTY = {"full": (), "middle-empty": (1,), "all-empty": (0, 1, 2)}


def assert_post_case_is_not_vacuous(nc, variant, thr, k, truncates, pred, shapes, full_ref):
    """from the oracle's decode and its un-truncated survivors (`full_ref`: O.postprocess with no top-k cut)"""
    survivors = [len(r["scores"]) for r in full_ref]
    for i, c in enumerate(survivors):
        assert (c == 0) == (i in POST_EMPTY[variant]), (variant, survivors)
    if truncates:
        assert min(survivors) > k, f"nc={nc}: top-k {k} cuts nothing ({survivors})"
    hot = hottest_pixel_records(pred, shapes, thr)
    if nc >= 166 and variant == "full":
        # 3 * nc records is all a pixel can pass: 498 at nc = 166 (below the 512-record buffer whatever the logits), more than DEC_BUF from nc = 171 on
        assert hot == 3 * nc and (hot > DEC_BUF or nc < 171), (nc, hot)
    return survivors, hot
