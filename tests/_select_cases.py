"""Shared by tests/test_select_sort.py (CPU: the cases' own conditions) and tests/test_select_sort_gpu.py (the real kernels): inputs that steer the per-image
score-prefix selection and the two per-image sorts of the detection post-process (yolort_amd/csrc/postprocess.hip: select_prefix_kernel, the sel_* multi-block
kernels with their refinement ladder, rank_image_kernel / scatter_ranks_kernel, sort_image_kernel) path by path, and the conditions, computed from the oracle alone,
under which a case says anything.

Score control.  One level (stride 8, 48 x 48 cells, 3 anchors).  The objectness logit is 20 everywhere: sigmoid is exactly 1.0 in fp32 from 17.4 on, so a score IS the
class sigmoid.  The class logit of a pair that is no candidate is -20 (score 2e-9, far below the threshold 1e-4).  So a case fixes the exact number of records of every
image and the exact score of every (anchor, class) pair.  Every case is checked against one rule with the oracle's own decode: two unequal scores differ by at least
1e-5 relative (five times the score tolerance of the post-process tests), so the order is decided by exact ties (candidate index, then label) or by gaps that no
rounding of expf can flip.

Boxes are anchor sized and centred on their cells (box logits randn * 0.05); the anchor size `aw` is the knob for how deep the suppression reaches."""
import functools

import numpy as np
import torch

# restated from postprocess.hip; tests/test_select_sort.py checks them against its text
RANK_MAX = 6144        # records of an image the ranking sort takes; a refined selection stops as soon as it fits
SEL_SLICE = 16384      # records per block of the multi-block selection
SEL_BINS = 4096        # linear score bins of the selection's first level
IMG_SORT_MAX = 16384   # LDS run of sort_image_kernel under YMI_POST_EXACT_FULL (half of it by default)


def sel_t(k):
    """records the selection aims for"""
    return max(4 * k, 4096)


def is_cut(count, k):
    return count > sel_t(k) + sel_t(k) // 2


H = W = 48
STRIDE = 8
ANCHORS_PER_IMAGE = 3 * H * W
THR, NMS_THR = 1e-4, 0.45
OBJ_LOGIT, OFF_LOGIT, ONE_LOGIT = 20.0, -20.0, 20.0
MIN_GAP = 1e-5
PATTERNS = ("spread", "fat-bin", "all-equal", "two-valued", "top-and-bottom", "sparse")


def pattern_scores(pattern, count):
    """the `count` scores of a pattern, best first, as float64 (1.0 stands for the class logit 20)"""
    j = np.arange(count, dtype=np.float64)
    if pattern == "spread":            # distinct, 3e-5 relative apart: ~7 records per linear bin at the top, a plain cut
        return 0.9 * np.exp(-3e-5 * j)
    if pattern == "sparse":
        return 0.8 * np.exp(-1e-3 * j)
    if pattern == "all-equal":
        return np.full(count, 1.0 / (1.0 + np.exp(-1.0)))
    if pattern == "two-valued":        # 1500 records of the upper value: sel_t falls inside the ties of the lower one
        return np.where(j < 1500, 1.0 / (1.0 + np.exp(-2.0)), 1.0 / (1.0 + np.exp(-0.5)))
    if pattern == "top-and-bottom":    # 3000 records of exactly 1.0 (bin 0), the rest one step above the threshold (bin 4095: scores below 1 / 4096)
        low = 1.1e-4 * np.exp(3e-5 * (count - 1 - j))
        assert low.max() < 2.4e-4
        return np.where(j < 3000, 1.0, low)
    if pattern == "fat-bin":
        # 16 values inside linear bin 2048 (scores in (0.499756, 0.5]), 1.2e-5 apart, each repeated: 6400 records where the image is large enough for it, with 2000
        # distinct better scores before the bin and distinct worse scores behind it; a smaller image is the bin alone
        values = 0.49978 + 1.2e-5 * np.arange(15, -1, -1, dtype=np.float64)
        if count < 9000:
            return values[(j * 16 // count).astype(np.int64)]
        top, rep = 2000, 400
        s = np.empty(count, np.float64)
        s[:top] = 0.95 * np.exp(-2e-5 * j[:top])
        s[top: top + 16 * rep] = np.repeat(values, rep)
        s[top + 16 * rep:] = 0.45 * np.exp(-3e-5 * np.arange(count - top - 16 * rep, dtype=np.float64))
        return s
    raise KeyError(pattern)


def image_logits(pattern, count, nc, seed):
    """(3, H, W, nc + 5) head output of one image: `count` candidate (anchor, class) pairs at seeded places, the pattern's scores dealt to them at random"""
    rng = np.random.default_rng(1000 * PATTERNS.index(pattern) + count + nc + seed)
    assert 0 < count <= ANCHORS_PER_IMAGE * nc
    s = pattern_scores(pattern, count)
    logit = np.where(s >= 1.0, ONE_LOGIT, np.log(np.minimum(s, 0.999) / (1.0 - np.minimum(s, 0.999))))
    cls = np.full(ANCHORS_PER_IMAGE * nc, OFF_LOGIT, np.float64)
    where = rng.permutation(ANCHORS_PER_IMAGE * nc)[:count]
    cls[where] = logit[rng.permutation(count)]
    out = torch.zeros(3, H, W, nc + 5, dtype=torch.float32)
    out[..., :4] = torch.from_numpy(rng.standard_normal((3, H, W, 4)).astype(np.float32) * np.float32(0.05))
    out[..., 4] = OBJ_LOGIT
    out[..., 5:] = torch.from_numpy(cls.astype(np.float32)).view(3, H, W, nc)   # anchor index = (a * H + y) * W + x, the oracle's order
    return out


class Data:
    """a batch: per image (pattern, record count), one class count and one anchor size.  `seeds`: per image, default its index (equal seeds: equal images)"""

    def __init__(self, name, images, nc, aw, seeds=None):
        self.name, self.images, self.nc, self.aw = name, tuple(images), nc, float(aw)
        self.n = len(self.images)
        self.seeds = tuple(range(self.n)) if seeds is None else tuple(seeds)
        self.counts = [c for _, c in self.images]
        self.strides = [STRIDE]
        self.anchors = [[self.aw, self.aw, 1.1 * self.aw, 0.9 * self.aw, 0.9 * self.aw, 1.1 * self.aw]]

    def heads(self):
        return [torch.stack([image_logits(p, c, self.nc, s) for (p, c), s in zip(self.images, self.seeds)])]

    def __repr__(self):
        return self.name


def _oracle():
    from oracle import yolov5_oracle as O
    return O


@functools.lru_cache(maxsize=None)
def _reference(data, agnostic):
    O = _oracle()
    pred = O.decode(data.heads(), data.strides, data.anchors)
    assert bool((pred[..., 4] == 1.0).all()), "the objectness is not exactly 1.0"
    images, done = [], {}
    for i in range(data.n):
        if (data.images[i], data.seeds[i]) in done:   # an equal image: the same (read-only) result
            images.append(done[data.images[i], data.seeds[i]])
            continue
        p = pred[i]
        scores = p[:, 5:] * p[:, 4:5]
        cx, cy, w, h = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
        boxes = torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)
        inds, labels = torch.where(scores > THR)
        b, s = boxes[inds], scores[inds, labels]
        kept = O.batched_nms(b, s, torch.zeros_like(labels) if agnostic else labels, NMS_THR)
        sn = s.numpy()
        order = np.lexsort((np.arange(len(sn)), -sn.astype(np.float64)))   # score descending, ties by candidate order (anchor, then class)
        rank = np.empty(len(sn), np.int64)
        rank[order] = np.arange(len(sn))
        images.append(dict(scores=s[kept], labels=labels[kept], boxes=b[kept], all_scores=sn, kept_rank=rank[kept.numpy()]))
        done[data.images[i], data.seeds[i]] = images[-1]
    return images


def reference(data, agnostic=False):
    """per image, from the oracle alone and WITHOUT a top-k cut (the cut is a slice: box_head.py:423): scores / labels / boxes of every survivor in output order,
    `all_scores` of every candidate in candidate order, `kept_rank` = rank of every survivor in the full score order.  Computed once per batch, never modified."""
    return _reference(data, bool(agnostic))


def top_k(ref, k):
    return [{key: r[key][:k] for key in ("scores", "labels", "boxes")} for r in ref]


def min_relative_gap(all_scores):
    u = np.unique(all_scores.astype(np.float64))
    return np.inf if len(u) < 2 else float(((u[1:] - u[:-1]) / u[1:]).min())


def crossing_bin_count(all_scores, k):
    """records of the best linear bins that together reach sel_t (the first level's selection, in the kernel's fp32 arithmetic); more than RANK_MAX: the bin is FAT"""
    b = np.clip(((np.float32(1.0) - all_scores.astype(np.float32)) * np.float32(SEL_BINS)).astype(np.int64), 0, SEL_BINS - 1)
    cum = np.cumsum(np.bincount(b, minlength=SEL_BINS))
    return int(cum[np.searchsorted(cum, sel_t(k))])


def stats(data, k, agnostic=False):
    """per image: records, survivors within the top sel_t and within the top max(RANK_MAX, sel_t) records, rank of the last returned survivor (-1: none)"""
    out = []
    for r in reference(data, agnostic):
        kr = r["kept_rank"]
        last = int(kr[min(k, len(kr)) - 1]) if len(kr) else -1
        out.append(dict(count=len(r["all_scores"]), survivors=len(kr), in_sel=int(np.searchsorted(kr, sel_t(k))), in_max=int(np.searchsorted(kr, max(RANK_MAX, sel_t(k)))),
                        last_rank=last))
    return out


def assert_case(data, k, kind, agnostic=False, verbose=True):
    """the conditions under which the case (`kind`: "suffices", "short" or None for a batch without a cut image) says anything; -> stats"""
    ref = reference(data, agnostic)
    st = stats(data, k, agnostic)
    for i, (r, s, (pattern, count)) in enumerate(zip(ref, st, data.images)):
        assert s["count"] == count, f"{data} image {i}: {s['count']} candidates, {count} wanted"
        gap = min_relative_gap(r["all_scores"])
        assert gap >= MIN_GAP, f"{data} image {i}: two unequal scores are {gap:.3g} apart"
        if verbose:
            print(f"{data} k={k} image {i} ({pattern}): candidates {s['count']} cut {is_cut(count, k)} survivors {s['survivors']} within sel_t={sel_t(k)}: {s['in_sel']} "
                  f"within {max(RANK_MAX, sel_t(k))}: {s['in_max']} last returned survivor at rank {s['last_rank']}")
        if not is_cut(count, k):
            continue
        if pattern in ("fat-bin", "all-equal", "two-valued", "top-and-bottom") and sel_t(k) <= RANK_MAX:
            assert crossing_bin_count(r["all_scores"], k) > RANK_MAX, f"{data} image {i}: the crossing bin is not fat"
        if pattern == "spread" and sel_t(k) == SEL_BINS:   # (a larger target leaves the ranking sort no slack: every cut is refined)
            assert crossing_bin_count(r["all_scores"], k) <= RANK_MAX, f"{data} image {i}: the cut is not plain"
        if kind == "suffices":
            assert s["in_sel"] >= k and s["last_rank"] >= sel_t(k) // 2, f"{data} k={k} image {i}: {s}"
        elif kind == "short":
            assert s["in_max"] < k, f"{data} k={k} image {i}: {s}"
    cut = [is_cut(c, k) for c in data.counts]
    assert any(cut) == (kind is not None), (data, k, kind)
    return st


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """a batch under one detections_per_img.  kind: "suffices" (every cut image has >= k survivors within its top sel_t records and its last returned survivor ranks
    beyond sel_t / 2: a record lost or duplicated deep in the selection changes the output), "short" (fewer than k survivors within the top max(RANK_MAX, sel_t):
    any legal selection raises YMI_STATUS_PREFIX_SHORT) or None (no image is cut: the batch is small, or `exact` = YMI_POST_EXACT_FULL)"""

    def __init__(self, data, k, kind, agnostic=False, exact=False):
        self.data, self.k, self.kind, self.agnostic, self.exact = data, k, kind, agnostic, exact
        self.name = f"{data.name}-k{k}" + ("-agnostic" if agnostic else "") + ("-exact" if exact else "")

    def cut(self):
        return [not self.exact and is_cut(c, self.k) for c in self.data.counts]

    def __repr__(self):
        return self.name


SPARSE = ("sparse", 300)
DATA, CASES = {}, {}


def _data(pattern, count, nc, aw):
    name = f"{pattern}-{count}-aw{aw:g}"
    if name not in DATA:
        DATA[name] = Data(name, [(pattern, count), SPARSE], nc, aw)
    return DATA[name]


def _case(data, k, kind, **kw):
    c = Case(data, k, kind, **kw)
    return CASES.setdefault(c.name, c)


# anchor sizes were searched so that the ORACLE's result meets the case's condition (tests/test_select_sort.py asserts it); nothing here looks at the kernels' output.
# One crowded image followed by a sparse one (never cut: it checks the compact offset behind a cut image), k = 300 (sel_t = 4096):
PATTERN_CASES = [
    _case(_data("spread", 6144, 4, 110), 300, None),                  # 1.5 * sel_t: not cut
    _case(_data("spread", 6145, 4, 110), 300, "suffices"),            # cut
    _case(_data("spread", 16384, 4, 110), 300, "suffices"),           # one full slice
    _case(_data("spread", 16385, 4, 110), 300, "suffices"),           # ... and one record of the next
    _case(_data("spread", 27648, 4, 110), 300, "suffices"),           # the whole map, nc = 4
    _case(_data("spread", 55296, 8, 158), 300, "suffices"),           # the whole map, nc = 8: four slices, the last one ragged
    _case(_data("fat-bin", 6145, 4, 110), 300, "suffices"),
    _case(_data("fat-bin", 16385, 4, 110), 300, "suffices"),
    _case(_data("fat-bin", 55296, 8, 158), 300, "suffices"),
    _case(_data("all-equal", 16384, 4, 100), 300, "suffices"),
    _case(_data("all-equal", 27648, 4, 80), 300, "suffices"),
    _case(_data("two-valued", 6145, 4, 112), 300, "suffices"),
    _case(_data("two-valued", 27648, 4, 110), 300, "suffices"),
    _case(_data("top-and-bottom", 16385, 4, 113), 300, "suffices"),
    _case(_data("spread", 27648, 4, 400), 300, "short"),
    _case(_data("all-equal", 27648, 4, 180), 300, "short"),
    _case(_data("fat-bin", 55296, 8, 220), 300, "short"),
]

# detections_per_img -> anchor size on the whole nc = 8 map: sel_t = 4096, 6000, 6144, 6148 (the first above RANK_MAX), 8000, 8192 (one run of sort_image_kernel),
# 8196 and 12000 (two runs)
K_SWEEP = {300: 158, 1500: 56, 1536: 56, 1537: 56, 2000: 48, 2048: 48, 2049: 48, 3000: 40}
K_CASES = [_case(_data("spread", 55296, 8, aw), k, "suffices") for k, aw in K_SWEEP.items()]
# sel_t = 6148 is four records past RANK_MAX: a selection that lost four records of 6148 still returns the right detections about one time in three.  Six EQUAL crowded
# images (and the sparse one) lose or keep their records independently
DATA["spread-55296-aw56-x6"] = Data("spread-55296-aw56-x6", [("spread", 55296)] * 6 + [SPARSE], 8, 56, seeds=[0] * 6 + [1])
K_EQUAL_IMAGES = _case(DATA["spread-55296-aw56-x6"], 1537, "suffices")
K_SHORT = _case(_data("spread", 55296, 8, 60), 2000, "short")

# YMI_POST_EXACT_FULL: no selection; 6144 records take the ranking sort, 6145 one LDS run of sort_image_kernel, 16384 / 16385 one / two runs, 55296 four (ragged last)
EXACT_CASES = [_case(_data(p, c, nc, 110), 300, None, exact=True) for p, c, nc in (("spread", 6144, 4), ("spread", 6145, 4), ("all-equal", 16384, 4), ("fat-bin", 16385, 4),
                                                                                  ("spread", 55296, 8))]
DATA["rank-then-runs"] = Data("rank-then-runs", [("spread", 6144), ("two-valued", 16385)], 4, 110)
DATA["runs-then-rank"] = Data("runs-then-rank", [("two-valued", 16385), ("spread", 6144)], 4, 110)
EXACT_MIXED = [_case(DATA["rank-then-runs"], 300, None, exact=True), _case(DATA["runs-then-rank"], 300, None, exact=True)]

# YMI_POST_AGNOSTIC (P keys without label bits): a fat bin, and sel_t = 8196 (two runs)
AGNOSTIC_CASES = [_case(_data("fat-bin", 55296, 8, 56), 300, "suffices", agnostic=True), _case(_data("spread", 55296, 8, 12), 2049, "suffices", agnostic=True)]

# image 0 cut, image 1 sparse (left alone), image 2 crowded but not above 1.5 * sel_t (not cut)
DATA["cut-sparse-uncut"] = Data("cut-sparse-uncut", [("spread", 27648), SPARSE, ("two-valued", 6144)], 4, 110)
MIXED3 = _case(DATA["cut-sparse-uncut"], 300, "suffices")
# 32 images (the one-block form by default): images 0 and 31 crowded with different patterns, the others sparse
DATA["batch-32"] = Data("batch-32", [("fat-bin", 16385)] + [SPARSE] * 30 + [("all-equal", 16384)], 4, 110)
BATCH32 = _case(DATA["batch-32"], 300, "suffices")

ALL_CASES = list(CASES.values())
