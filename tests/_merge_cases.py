"""Shared by tests/test_merge_nms.py (CPU: host logic, the yardstick's own checks, the simulator) and tests/test_merge_nms_gpu.py (the real kernels): the yardstick of
MERGE-NMS (include/yolort_amd.h YMI_POST_MERGE / YMI_POST_MERGE_KEEP_SINGLE; Python `merge=True`, `merge_redundant=`), the case table and the comparison.

The yardstick.  ultralytics keeps `merge = False` as a local constant of non_max_suppression, so no reference run can produce a golden: `merge_reference` is a float64 numpy
restatement of yolort/v5/utils/general.py:604-613 on top of the ORACLE's candidates and keep lists (O.decode, the threshold / best-class / class-filter rules of
_classes_cases.filtered_reference, O.batched_nms), with the three documented differences of the header (unshifted same-class boxes, no max_nms cut, the zero-weight
rule).  Per image of n candidates, merged iff 1 < n < 3000: the kept list is cut to k FIRST; the contributors of a kept record are the candidates of its label (any label
when agnostic) whose IoU with it is > nms; the merged box is sum(score * box) / sum(score) in float64; a record with <= 1 contributors is dropped unless keep_single.

Tolerance of a merged coordinate (derived, not tuned): m rounded products summed in any order, divided by a sum of m terms, one division:
(2 m + 3) * 2^-24 * max |coordinate of the contributors|.  EXACT cases (small-integer boxes, scores 1, 0.5, 0.25 or 0 from the logit palette of _head_cases: 20 -> sigmoid
1.0, 0 -> 0.5, <= -104 -> 0) have every partial sum exact in fp32, so the output must equal np.float32(num) / np.float32(den) bit for bit whatever the order.

Every case keeps all pair IoUs it decides on at least 1e-4 away from nms, or on values exact in fp32 that fp32 and float64 decide alike (`merge_reference` asserts it), so
the contributor sets are unambiguous."""
import functools

import numpy as np
import torch

import _agnostic_cases as A
import _classes_cases as K

POST_MERGE, POST_MERGE_KEEP_SINGLE = 16, 32   # include/yolort_amd.h (restated so that a missing constant fails a test, not the collection)
POST_CLASS_FILTER, POST_AGNOSTIC, POST_BEST_CLASS, POST_EXACT_FULL = 8, 4, 2, 1
MERGE_MAX_N = 3000
MRG_WAVES = 16        # waves of merge_gather_kernel's workgroup (postprocess.hip): kept records are dealt to them round-robin
IOU_MARGIN = 1e-4
F32 = np.float32


def _oracle():
    from oracle import yolov5_oracle as O
    return O


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------------------------------------
def candidates(p, thr, best, classes):
    """one image of the oracle's decode -> (boxes, scores, labels) in candidate order (anchor ascending, class ascending), as _classes_cases.filtered_reference takes them"""
    scores = p[:, 5:] * p[:, 4:5]
    nc = scores.shape[1]
    allowed = torch.ones(nc, dtype=torch.bool) if classes is None else torch.zeros(nc, dtype=torch.bool)
    if classes is not None and len(classes):
        allowed[torch.tensor(sorted(classes), dtype=torch.long)] = True
    cx, cy, w, h = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    boxes = torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)
    if best:
        conf, j = scores.max(1)
        keep = conf > thr
        b, s, lab = boxes[keep], conf[keep], j[keep]
    else:
        inds, lab = torch.where(scores > thr)
        b, s = boxes[inds], scores[inds, lab]
    sel = allowed[lab]
    return b[sel], s[sel], lab[sel]


def iou64(box, boxes):
    """float64 IoU of one box with many (torchvision's expression); 0 / 0 = NaN, which never passes a threshold"""
    box, boxes = box.astype(np.float64), boxes.astype(np.float64)
    x1, y1 = np.maximum(box[0], boxes[:, 0]), np.maximum(box[1], boxes[:, 1])
    x2, y2 = np.minimum(box[2], boxes[:, 2]), np.minimum(box[3], boxes[:, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    a = (box[2] - box[0]) * (box[3] - box[1])
    b = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (a + b - inter)


def iou32(box, boxes):
    """the same in fp32, operation for operation (postprocess.hip iou_gt)"""
    box, boxes = box.astype(F32), boxes.astype(F32)
    x1, y1 = np.maximum(box[0], boxes[:, 0]), np.maximum(box[1], boxes[:, 1])
    x2, y2 = np.minimum(box[2], boxes[:, 2]), np.minimum(box[3], boxes[:, 3])
    inter = (np.maximum(F32(0), x2 - x1) * np.maximum(F32(0), y2 - y1)).astype(F32)
    a = F32((box[2] - box[0]) * (box[3] - box[1]))
    b = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (inter / ((a + b).astype(F32) - inter).astype(F32)).astype(F32)


def merge_image(b, s, lab, kept, nms, agnostic, keep_single):
    """general.py:604-613 on one image's candidates (numpy, candidate order) and its kept list ALREADY cut to k -> dict(boxes float64, scores, labels, m, tol, num, den,
    moved, kept_before, merged flag).  Asserts the IoU margin on every pair it decides."""
    n = len(s)
    if not 1 < n < MERGE_MAX_N:
        return dict(boxes=b[kept].astype(np.float64), scores=s[kept], labels=lab[kept], m=np.full(len(kept), -1), tol=np.zeros((len(kept), 4)), merged=False,
                    kept_before=len(kept), dropped=0, moved=np.zeros(len(kept)), num=None, den=None)
    out_b, out_m, out_tol, out_num, out_den, moved, live = [], [], [], [], [], [], []
    nms32 = F32(nms)
    for i in kept:
        iou = iou64(b[i], b)
        close = np.abs(iou - float(nms32)) < IOU_MARGIN   # (NaN compares False)
        if not agnostic:
            close &= lab == lab[i]                        # a pair of different labels is not decided by its IoU
        if close.any():   # only values exact in fp32 that both precisions decide alike may sit on the threshold
            i32 = iou32(b[i], b)
            assert (i32[close].astype(np.float64) == iou[close]).all() and ((i32[close] > nms32) == (iou[close] > float(nms32))).all(), \
                f"a pair IoU within {IOU_MARGIN} of the threshold: {iou[close]}"
        with np.errstate(invalid="ignore"):
            mask = iou > float(nms32)
        if not agnostic:
            mask &= lab == lab[i]
        m = int(mask.sum())
        w = s[mask].astype(np.float64)
        den = w.sum()
        num = (w[:, None] * b[mask].astype(np.float64)).sum(0) if m else np.zeros(4)
        box = num / den if den > 0 else b[i].astype(np.float64)   # the zero-weight rule: the NMS coordinates stay
        out_num.append(num if den > 0 else None), out_den.append(den)
        out_b.append(box), out_m.append(m)
        out_tol.append(np.full(4, (2 * m + 3) * 2.0 ** -24 * (np.abs(b[mask]).max() if m else 0.0)))
        moved.append(np.abs(box - b[i].astype(np.float64)).max())
        live.append(keep_single or m > 1)
    live = np.array(live, bool) if len(kept) else np.zeros(0, bool)
    sel = np.array(kept, np.int64)[live]
    pick = lambda lst: [x for x, f in zip(lst, live) if f]
    return dict(boxes=np.array(pick(out_b), np.float64).reshape(-1, 4), scores=s[sel], labels=lab[sel], m=np.array(pick(out_m), np.int64),
                tol=np.array(pick(out_tol), np.float64).reshape(-1, 4), merged=True, kept_before=len(kept), dropped=int((~live).sum()),
                moved=np.array(pick(moved), np.float64), num=pick(out_num), den=pick(out_den))


def oracle_candidates(pred, thr, best=False, classes=None):
    """per image (boxes, scores, labels) as numpy, in RANK order: score descending, ties in candidate order (the order of G)"""
    out = []
    for p in pred:
        b, s, lab = candidates(p, thr, best, classes)
        order = torch.sort(s, descending=True, stable=True)[1]
        out.append((b[order].numpy(), s[order].numpy(), lab[order].numpy()))
    return out


def merge_reference(cands, nms, k, agnostic=False, merge=True, keep_single=False):
    """cands: per image (boxes, scores, labels) in rank order -> per image the dict of merge_image (merge=False: the plain top-k, `merged` False everywhere).  The keep list
    is the oracle's: O.batched_nms on these candidates (labels zeroed for the call when agnostic), cut to k"""
    O = _oracle()
    out = []
    for bn, sn, ln in cands:
        b, s, lab = torch.from_numpy(np.ascontiguousarray(bn)), torch.from_numpy(np.ascontiguousarray(sn)), torch.from_numpy(np.ascontiguousarray(ln))
        kept = O.batched_nms(b, s, torch.zeros_like(lab) if agnostic else lab, nms)[:k].numpy() if len(sn) else np.zeros(0, np.int64)
        if merge:
            r = merge_image(bn, sn, ln, kept, nms, agnostic, keep_single)
        else:
            r = merge_image(bn[:0], sn[:0], ln[:0], [], nms, agnostic, keep_single)
            r.update(boxes=bn[kept].astype(np.float64), scores=sn[kept], labels=ln[kept], tol=np.zeros((len(kept), 4)), m=np.full(len(kept), -1), kept_before=len(kept),
                     moved=np.zeros(len(kept)))
        r["n"] = len(sn)
        out.append(r)
    return out


def operand_candidates(out):
    """the candidates as THE LIBRARY decoded them: the outputs of a run without the merge flag, nms_thresh = 1.0 (an IoU is never > 1: nothing is suppressed) and
    k >= every count -- all candidates of an image in rank order.  The merge arithmetic is then judged on its own operands (the decode's expf rounding, which the existing
    post-process tests allow for, does not enter the bound); assert_operands_match_oracle ties them to the oracle"""
    res = []
    for i in range(len(out["count"])):
        c = int(out["count"][i])
        res.append((out["boxes"][i, :c].numpy().copy(), out["scores"][i, :c].numpy().copy(), out["labels"][i, :c].numpy().copy()))
    return res


def assert_operands_match_oracle(cands, ref_cands, exact=False):
    """count, labels and order exact; scores and boxes to the rounding of expf (the constants of _head_cases.assert_equals_oracle), bit for bit in exact cases"""
    for i, ((b, s, lab), (rb, rs, rl)) in enumerate(zip(cands, ref_cands)):
        assert len(s) == len(rs), (i, len(s), len(rs))
        np.testing.assert_array_equal(lab, rl)
        if exact:
            np.testing.assert_array_equal(s, rs), np.testing.assert_array_equal(b, rb)
        else:
            np.testing.assert_allclose(s, rs, rtol=2e-6, atol=1e-7), np.testing.assert_allclose(b, rb, rtol=1e-5, atol=1e-4)


def assert_matches(got, ref, fill, exact=False, what=""):
    """counts, labels, order and scores exact (the reference is built on operands that are bit-identical to the run's own); merged boxes within the derived tolerance
    (2 m + 3) * 2^-24 * max |coordinate of the contributors| of the float64 value -- 0 for a box that is not merged: bit-equal --, and in exact cases bit-equal to
    np.float32(num) / np.float32(den); nothing written past the counts"""
    for i, r in enumerate(ref):
        c = int(got["count"][i])
        assert c == len(r["scores"]), (what, i, c, len(r["scores"]))
        np.testing.assert_array_equal(got["labels"][i, :c].numpy(), r["labels"], err_msg=f"{what} image {i}")
        gs, gb = got["scores"][i, :c].numpy(), got["boxes"][i, :c].numpy()
        np.testing.assert_array_equal(gs, r["scores"], err_msg=f"{what} image {i}")
        err = np.abs(gb.astype(np.float64) - r["boxes"])
        assert (err <= r["tol"]).all(), (what, i, float((err - r["tol"]).max()), r["m"][np.argmax((err - r["tol"]).max(1))])
        if exact:
            for j in range(c):
                if r["merged"] and r["num"][j] is not None:
                    num, den = r["num"][j], r["den"][j]
                    assert (num.astype(F32) == num).all() and F32(den) == den, "the case is not exact"
                    np.testing.assert_array_equal(gb[j], num.astype(F32) / F32(den), err_msg=f"{what} image {i} detection {j}")
                else:
                    np.testing.assert_array_equal(gb[j], r["boxes"][j].astype(F32), err_msg=f"{what} image {i} detection {j}")
        assert (got["scores"][i, c:] == fill).all() and (got["labels"][i, c:] == int(fill)).all() and (got["boxes"][i, c:] == fill).all(), f"{what} image {i}: slots past the count were written"


# ---- lattice cases: boxes with small-integer coordinates, scores from the exact palette ------------------------------------------------------------------------------------
LAT_STRIDE = 2.0
BIG = [64.0, 64.0, 64.0, 64.0, 0.0, 8.0]     # anchors 0 and 1: 64 x 64 boxes (two per pixel), anchor 2: a zero-area box (width 0)
SMALL = [16.0, 16.0, 16.0, 16.0, 0.0, 8.0]   # the same with 16 x 16 boxes
HI, MID, OFF, ZERO = 20.0, 0.0, -20.0, -110.0      # logits: sigmoid exactly 1.0, exactly 0.5, "fails", exactly 0.0
LAT_THR = 0.2                                      # palette scores 1.0, 0.5 and 0.25 pass


def lattice_heads(n, h, w, nc, cells):
    """cells: (img, anchor, y, x, objectness logit, {class: logit}) -> reference-layout head outputs [(n, 3, h, w, nc + 5)]; box logits 0: the box of (anchor, y, x) is
    centred at ((x + 0.5) * 2, (y + 0.5) * 2) with the anchor's size -- integers; everything not listed fails (objectness and classes at -20)"""
    ho = torch.zeros(n, 3, h, w, nc + 5)
    ho[..., 4:] = OFF
    for img, a, y, x, obj, cls in cells:
        assert 0 <= y < h and 0 <= x < w, (y, x)
        ho[img, a, y, x, 4] = obj
        for c, v in cls.items():
            ho[img, a, y, x, 5 + c] = v
    return [ho]


def _cluster(img, cy, cx, m, cls=0, reach=5):
    """m boxes around pixel (cy, cx) within `reach` pixels in both axes, anchors 0 and 1.  64 x 64 boxes, reach 5 (10 units): IoU with the centre box >= 54 * 54 /
    (8192 - 54 * 54) = 0.553; 16 x 16 boxes, reach 1: >= 14 * 14 / (512 - 14 * 14) = 0.62 -- above 0.45 with a wide margin.  The centre box (anchor 0) scores 1.0 and is
    the only kept one; the others score 0.5 / 0.25 alternately"""
    cells, offs = [], [(dy, dx, a) for a in (0, 1) for dy in range(-reach, reach + 1) for dx in range(-reach, reach + 1)]
    offs.sort(key=lambda t: (abs(t[0]) + abs(t[1]) + t[2], t))
    assert m <= len(offs)
    for q, (dy, dx, a) in enumerate(offs[:m]):
        obj, cl = (HI, HI) if q == 0 else ((HI, MID) if q % 2 else (MID, MID))
        cells.append((img, a, cy + dy, cx + dx, obj, {cls: cl}))
    return cells


CONTRIBUTORS = (1, 2, 63, 64, 65, 130)
LATTICE_CASES = ("contributors", "many-kept", "short-k", "shared-box", "filtered", "zero-area", "zero-weight", "global")


@functools.lru_cache(maxsize=None)
def lattice_case(name):
    """-> dict(heads, strides, anchors, pred, nc, thr, nms, k, cap, flags, classes, n) of a named case; every one has exact operands"""
    O = _oracle()
    nc, thr, nms, k, flags, classes, anc = 2, LAT_THR, 0.45, 300, 0, None, BIG
    if name == "contributors":   # shape 1: image q has ONE kept cluster box with CONTRIBUTORS[q] contributors, and a lone box far away (dropped as redundant)
        n, h, w = len(CONTRIBUTORS), 60, 20
        cells = []
        for q, m in enumerate(CONTRIBUTORS):
            cells += _cluster(q, 8, 8, m) + [(q, 0, 52, 8, HI, {1: MID})]
    elif name == "many-kept":    # shape 2: 40 clusters of one, two or three 16 x 16 boxes, 16 units apart (disjoint): more kept records than the block has waves
        n, h, w, anc = 1, 44, 68, SMALL
        cells = []
        for c in range(40):
            cells += _cluster(0, 4 + 8 * (c // 8), 4 + 8 * (c % 8), 1 + c % 3, cls=c % 2, reach=1)
    elif name == "short-k":      # shape 3: k = 4 below the kept count 6; the second-ranked kept record is a lone box, so the count ends at 3
        n, h, w, k = 1, 120, 20, 4
        cells = _cluster(0, 8, 8, 3) + [(0, 0, 40, 8, HI, {0: MID})] + [(0, 0, 72, 8, MID, {0: MID}), (0, 1, 72, 8, MID, {0: MID})] + \
                [(0, 0, 104, 8 + d, MID, {1: MID}) for d in (0, 1)] + [(0, 1, 104, 2, MID, {0: MID})] + [(0, 1, 40, 2, MID, {1: MID}), (0, 1, 40, 3, MID, {1: MID})]
    elif name == "shared-box":   # shapes 5 / 6: anchors whose two classes both pass share a box: agnostic -> they contribute to each other; class-aware -> each is alone
        n, h, w = 2, 60, 20
        cells = [(0, 0, 8, 8, HI, {0: HI, 1: MID}), (0, 0, 40, 8, HI, {0: MID, 1: MID}), (0, 0, 40, 9, MID, {1: MID}),
                 (1, 0, 8, 8, HI, {0: MID, 1: HI}), (1, 1, 8, 9, HI, {0: HI}), (1, 0, 40, 8, MID, {0: MID})]
    elif name == "filtered":     # shape 7: class 1 boxes that would contribute under agnostic NMS are removed by the filter {0}
        n, h, w, classes, flags = 1, 60, 20, (0,), POST_CLASS_FILTER | POST_AGNOSTIC
        cells = [(0, 0, 8, 8, HI, {0: HI}), (0, 0, 8, 9, HI, {1: MID}), (0, 0, 40, 8, HI, {0: HI}), (0, 0, 40, 9, HI, {0: MID}), (0, 1, 40, 10, MID, {1: MID})]
    elif name == "zero-area":    # shape 8: anchor 2 has width 0: IoU with itself is 0 / 0 = NaN, no contributor at all
        n, h, w = 1, 60, 20
        cells = [(0, 2, 8, 8, HI, {0: HI}), (0, 2, 8, 9, HI, {0: MID})] + _cluster(0, 40, 8, 3)
    elif name == "zero-weight":  # shape 9: score_thresh < 0 and every score exactly 0: all 3 * h * w * nc pairs are candidates, every weight sum is 0
        n, h, w, thr, cells = 2, 4, 5, -1.0, []
    elif name == "global":       # shape 10: cand_cap / n < 64 -> the global radix sort; 8 images of at most 6 candidates, one of them empty
        n, h, w = 8, 40, 12
        cells = []
        for img in range(8):
            cells += _cluster(img, 8, 6, 1 + img % 4, cls=img % 2) + ([(img, 0, 30, 6, HI, {1: MID}), (img, 1, 30, 6, MID, {1: MID})] if img % 2 else [(img, 0, 30, 6, HI, {0: MID})])
        cells = [c for c in cells if c[0] != 5]
    else:
        raise KeyError(name)
    heads = lattice_heads(n, h, w, nc, cells)
    strides, anchors = [LAT_STRIDE], [list(anc)]
    if name == "zero-weight":
        heads[0][..., 4] = MID   # every anchor passes, with score 0.5 * 0
        heads[0][..., 5:] = ZERO
    pred = O.decode(heads, strides, anchors)
    cap = n * 48 if name == "global" else n * 4096
    return dict(name=name, heads=heads, strides=strides, anchors=anchors, pred=pred, nc=nc, thr=thr, nms=nms, k=k, cap=cap, flags=flags, classes=classes, n=n, exact=True)


@functools.lru_cache(maxsize=None)
def bounds_case():
    """shape 4: n = 0, 1, 2, 2999 and 3000 candidates in one batch (eligibility at both ends, an empty image, an image change): a 25 x 40 level, one class, every anchor
    of images 3 and 4 passes (3000 anchors; image 3 loses one).  Anchors 0 and 1 coincide (IoU 1), anchor 2 has width 0"""
    O = _oracle()
    n, h, w, nc = 5, 25, 40, 1
    ho = lattice_heads(n, h, w, nc, [(1, 0, 8, 8, HI, {0: HI}), (2, 0, 8, 8, HI, {0: HI}), (2, 1, 8, 9, HI, {0: MID})])[0]
    g = torch.Generator().manual_seed(5)
    for img in (3, 4):
        pick = torch.randint(0, 3, (3, h, w), generator=g)
        ho[img, ..., 4] = torch.where(pick == 0, torch.tensor(HI), torch.tensor(MID))
        ho[img, ..., 5] = torch.where(pick == 1, torch.tensor(HI), torch.tensor(MID))
    ho[3, 2, h - 1, w - 1, 4] = OFF
    strides, anchors = [LAT_STRIDE], [list(BIG)]
    heads = [ho]
    return dict(name="bounds", heads=heads, strides=strides, anchors=anchors, pred=O.decode(heads, strides, anchors), nc=nc, thr=LAT_THR, nms=0.45, k=300, cap=n * 4096, flags=0,
                classes=None, n=n, exact=True, counts=[0, 1, 2, MERGE_MAX_N - 1, MERGE_MAX_N])


TRUNC_THR = 0.01


@functools.lru_cache(maxsize=None)
def truncated_case():
    """shape 12: an image of 6300 candidates (a 30 x 35 level, two classes, every pair passes: more than 1.5 * 4096, so the score-prefix selection cuts it) next to a
    mergeable one.  The crowded image's scores are random (the prefix is cut by score bins), its boxes are the lattice's"""
    O = _oracle()
    n, h, w, nc = 2, 30, 35, 2
    ho = lattice_heads(n, h, w, nc, _cluster(1, 8, 8, 5) + [(1, 0, 25, 8, HI, {1: MID})])[0]
    g = torch.Generator().manual_seed(12)
    ho[0, ..., 4] = 6.0
    ho[0, ..., 5:] = torch.randn(3, h, w, nc, generator=g)
    strides, anchors = [LAT_STRIDE], [list(BIG)]
    heads = [ho]
    return dict(name="truncated", heads=heads, strides=strides, anchors=anchors, pred=O.decode(heads, strides, anchors), nc=nc, thr=TRUNC_THR, nms=0.45, k=10, cap=n * 8192, flags=0,
                classes=None, n=n, exact=False, counts=[3 * h * w * nc, 6])


# ---- general cases: the oracle's random heads (boxes and scores through expf) ------------------------------------------------------------------------------------------
GENERAL_RUNS = (   # (nc, variant, thr, k, best, agnostic, classes)
    (2, "full", 0.05, 300, False, False, None),
    (2, "full", 0.05, 300, False, True, None),
    (2, "full", 0.05, 7, False, False, None),
    (2, "full", 0.3, 300, True, False, None),
    (2, "middle-empty", 0.3, 300, False, True, None),
    (80, "full", 0.05, 300, False, True, K.SET_A),
)
GENERAL_NMS = 0.4   # (at 0.45 one same-label pair of the nc = 2 heads has IoU 0.45000946: inside the margin.  At 0.4 every run keeps the margin; merge_image asserts it)


def run_flags(best=False, agnostic=False, classes=None, keep_single=False, merge=True):
    return (POST_BEST_CLASS if best else 0) | (POST_AGNOSTIC if agnostic else 0) | (POST_CLASS_FILTER if classes is not None else 0) | \
           ((POST_MERGE | (POST_MERGE_KEEP_SINGLE if keep_single else 0)) if merge else 0)


def general_case(run):
    """a run of GENERAL_RUNS on the simulator's levels (the GPU suite uses the same inputs: one reference for both)"""
    nc, variant, thr, k, best, agnostic, classes = run
    heads, strides, anchors, pred = A.post_inputs(nc, variant, True)
    return dict(name=f"general-{nc}-{variant}-{thr}-{k}-{'best' if best else 'multi'}-{'agnostic' if agnostic else 'aware'}", heads=heads, strides=strides, anchors=anchors, pred=pred,
                nc=nc, thr=thr, nms=GENERAL_NMS, k=k, cap=3 * 4096, flags=run_flags(best, agnostic, classes, merge=False), classes=classes, n=heads[0].shape[0], exact=False)


def case_modes(case):
    """(best, agnostic) of a case's own flags"""
    return bool(case["flags"] & POST_BEST_CLASS), bool(case["flags"] & POST_AGNOSTIC)


def assert_not_vacuous(ref, what, want_move=True, want_drop=True):
    """from the yardstick alone: some image is merged and yields detections, some box moves by more than its tolerance, some record is dropped as redundant"""
    assert any(r["merged"] for r in ref), what
    assert sum(len(r["scores"]) for r in ref if r["merged"]) > 0, f"{what}: no merged image yields a detection"
    if want_move:
        assert any((r["moved"] > r["tol"].max(1) + 1e-3).any() for r in ref if r["merged"] and len(r["moved"])), f"{what}: no box moves"
    if want_drop:
        assert sum(r["dropped"] for r in ref if r["merged"]) > 0, f"{what}: nothing is dropped as redundant"


def same_detections(a, b):
    """do two reference lists describe the same detections (counts, labels, scores, boxes)"""
    return all(len(x["scores"]) == len(y["scores"]) and np.array_equal(x["labels"], y["labels"]) and np.array_equal(x["scores"], y["scores"]) and np.array_equal(x["boxes"], y["boxes"])
               for x, y in zip(a, b))
