"""Detection metrics on the host (numpy): COCO-style average precision without pycocotools.

`coco_ap` restates the published COCO detection protocol (AP averaged over IoU 0.50:0.05:0.95, 101-point interpolated
precision, greedy score-ordered matching per class and image) for box detections.  `DetectionEvaluator` offers the
update()/compute() surface of the reference's evaluator (yolort/data/coco_eval.py:28-120, which wraps pycocotools --
absent here) on in-memory ground truth: SURVEY.md 8f-4.  COCO's maxDets = 100 cap -- per (image, category), as pycocotools
applies it -- its exact threshold grid linspace(.5, .95, 10) and its small / medium / large area ranges (ignore semantics of
COCOeval.evaluateImg) are applied; crowd boxes are not modelled (the in-memory ground truth has none).  `update_from_slab`
feeds the evaluator from the fixed-shape detection slab the ranks all-gather (yolort_amd/dist.py), so every rank scores the
GLOBAL batch without the reference's pickle exchange (yolort/data/coco_eval.py:225-226 -> data/distributed.py:6-49).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np


def _iou_matrix(a, b):
    x1 = np.maximum(a[:, None, 0], b[None, :, 0]); y1 = np.maximum(a[:, None, 1], b[None, :, 1])
    x2 = np.minimum(a[:, None, 2], b[None, :, 2]); y2 = np.minimum(a[:, None, 3], b[None, :, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]); ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (aa[:, None] + ab[None, :] - inter + 1e-12)


COCO_IOU_THRS = np.linspace(0.5, 0.95, 10)   # pycocotools Params.iouThrs (np.arange(.5, .96, .05) drifts: 0.7000000000000001 ...)
COCO_MAX_DETS = 100
# pycocotools Params.areaRng / areaRngLbl (the reference's summary lines, yolort/data/coco_eval.py:86-218 -> COCOeval.summarize)
COCO_AREA_RNG = {"all": (0.0, 1e10), "small": (0.0, 32.0 ** 2), "medium": (32.0 ** 2, 96.0 ** 2), "large": (96.0 ** 2, 1e10)}


def _area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def _ap_per_threshold(scores, tps, igs, n_gt):
    """The accumulation of one class, shared by `coco_ap` and `GpuDetectionEvaluator`: `scores` (D) float64, `tps` / `igs` (D, T) bool in record order (image order,
    then score order within the image), `n_gt` > 0 non-ignored ground truths -> the 101-point interpolated AP per threshold (a list of T float64)."""
    order = np.argsort(-scores, kind="stable")   # stable: equal scores keep image order, like pycocotools' mergesort
    tps = tps[order].astype(np.float64)
    igs = igs[order]
    ap_t = []
    for ti in range(tps.shape[1]):
        keep = ~igs[:, ti]
        t_ = tps[keep, ti]
        ctp = np.cumsum(t_); cfp = np.cumsum(1.0 - t_)
        rec = ctp / n_gt; prec = ctp / np.maximum(ctp + cfp, 1e-12)
        prec = np.maximum.accumulate(prec[::-1])[::-1]   # the precision envelope: every value the maximum of itself and those behind it
        q = np.zeros(101)
        inds = np.searchsorted(rec, np.linspace(0, 1, 101), side="left")
        ok = inds < len(prec)
        q[ok] = prec[inds[ok]]
        ap_t.append(q.mean())
    return ap_t


def coco_ap(refs, dets, num_classes=80, thrs=None, max_dets=None, area_rng=None):
    """COCO-style AP@[.5:.95] (101-point interpolation, greedy score-ordered matching per class and image) of `dets`
    with the ORACLE's detections `refs` as ground truth -- the 'mAP vs ref' of SURVEY.md 8d.  Lists of per-image dicts
    of numpy arrays {boxes (n,4), scores (n), labels (n)}.

    `max_dets`: as pycocotools applies maxDets -- PER (image, category): `dt = _dts[imgId, catId]` sorted by score, cut at
    `[0:maxDet]` (COCO: 100); None scores everything handed in (the bench's mAP-vs-ref compares full 300-detection outputs).
    `area_rng` = (lo, hi): COCO's area ranges -- ground truth outside the range is IGNORED (a detection matched to it counts neither
    as true nor as false positive; non-ignored ground truth is preferred in the matching), and so is an unmatched detection whose
    own area is outside the range (pycocotools COCOeval.evaluateImg)."""
    thrs = COCO_IOU_THRS if thrs is None else np.asarray(thrs)
    aps = []
    for c in range(num_classes):
        n_gt = 0
        recs = []   # (score, tp flags per threshold, ignore flags per threshold)
        for r, d in zip(refs, dets):
            gb = r["boxes"][r["labels"] == c]
            g_ign = np.zeros(len(gb), bool)
            if area_rng is not None and len(gb):
                ga = _area(gb)
                g_ign = (ga < area_rng[0]) | (ga > area_rng[1])
            go = np.argsort(g_ign, kind="stable")            # non-ignored ground truth first
            gb, g_ign = gb[go], g_ign[go]
            n_gt += int((~g_ign).sum())
            m = d["labels"] == c
            db, ds = d["boxes"][m], d["scores"][m]
            order = np.argsort(-ds, kind="stable")
            if max_dets is not None:
                order = order[:max_dets]                     # maxDets per (image, category)
            db, ds = db[order], ds[order]
            iou = _iou_matrix(db, gb) if len(db) and len(gb) else np.zeros((len(db), len(gb)))
            d_out = np.zeros(len(db), bool)
            if area_rng is not None and len(db):
                da = _area(db)
                d_out = (da < area_rng[0]) | (da > area_rng[1])
            tp = np.zeros((len(db), len(thrs)), bool)
            ig = np.zeros((len(db), len(thrs)), bool)
            for ti, t in enumerate(thrs):
                used = np.zeros(len(gb), bool)
                for i in range(len(db)):
                    best, bj = min(t, 1 - 1e-10), -1
                    for j in range(len(gb)):
                        if used[j]:
                            continue
                        if bj > -1 and not g_ign[bj] and g_ign[j]:
                            break                             # matched to real ground truth: ignored boxes are not considered
                        if iou[i, j] < best:
                            continue
                        best, bj = iou[i, j], j
                    if bj >= 0:
                        used[bj] = True
                        tp[i, ti] = not g_ign[bj]
                        ig[i, ti] = g_ign[bj]
                    else:
                        ig[i, ti] = d_out[i]
            recs += [(float(ds[i]), tp[i], ig[i]) for i in range(len(db))]
        if n_gt == 0:
            continue
        if not recs:
            aps.append(0.0)
            continue
        ap_t = _ap_per_threshold(np.array([x[0] for x in recs], np.float64), np.stack([x[1] for x in recs]), np.stack([x[2] for x in recs]), n_gt)
        aps.append(float(np.mean(ap_t)))
    return float(np.mean(aps)) if aps else None


class DetectionEvaluator:
    """Accumulates detections and ground truth per image; compute() returns COCO-style numbers in the 0-100 range
    (like the reference: yolort/data/coco_eval.py:31-34), -1 when nothing can be scored."""

    def __init__(self, num_classes: int = 80, max_dets: Optional[int] = COCO_MAX_DETS):
        self.num_classes = num_classes
        self.max_dets = max_dets   # COCO evaluates the top-100 detections per (image, category)
        self._preds: List[Dict[str, np.ndarray]] = []
        self._gts: List[Dict[str, np.ndarray]] = []

    @staticmethod
    def _np(d, keys) -> Dict[str, np.ndarray]:
        out = {}
        for k in keys:
            v = d[k]
            if hasattr(v, "detach"):
                v = v.detach().float().cpu().numpy() if k != "labels" else v.detach().cpu().numpy()
            out[k] = np.asarray(v)
        return out

    def update(self, preds: Sequence[Dict], targets: Sequence[Dict]) -> None:
        """preds: the model's List[Dict{boxes, scores, labels}]; targets: List[Dict{boxes, labels}] (xyxy, same image order)"""
        if len(preds) != len(targets):
            raise ValueError("one target per prediction is required")
        for p, t in zip(preds, targets):
            self._preds.append(self._np(p, ("boxes", "scores", "labels")))
            g = self._np(t, ("boxes", "labels"))
            g["scores"] = np.ones(len(g["labels"]), np.float32)
            self._gts.append(g)

    def update_from_slab(self, slab, targets: Sequence[Dict]) -> None:
        """slab = (boxes (N,K,4), scores (N,K), labels (N,K), counts (N)) of the GLOBAL batch in rank order -- what
        `PendingDetections.gathered()` / `dist.all_gather_slab` return; targets: ground truth of the same N images in the same order"""
        boxes, scores, labels, counts = [t.detach().cpu() if hasattr(t, "detach") else t for t in slab]
        cl = [int(c) for c in counts]
        if any(c < 0 for c in cl):
            raise ValueError("the slab still holds a stale shard: take PendingDetections.gathered() (it resolves the second round) first")
        self.update([{"boxes": boxes[i, :c], "scores": scores[i, :c], "labels": labels[i, :c]} for i, c in enumerate(cl)], targets)

    def merge(self, other: "DetectionEvaluator") -> None:
        """fold in another rank's accumulator (ranks own disjoint image shards)"""
        self._preds += other._preds
        self._gts += other._gts

    def compute(self) -> Dict[str, float]:
        if not self._gts:
            return {"AP": -1.0, "AP50": -1.0, "AP75": -1.0, "APs": -1.0, "APm": -1.0, "APl": -1.0}
        ap = coco_ap(self._gts, self._preds, self.num_classes, max_dets=self.max_dets)
        ap50 = coco_ap(self._gts, self._preds, self.num_classes, thrs=np.array([0.5]), max_dets=self.max_dets)
        ap75 = coco_ap(self._gts, self._preds, self.num_classes, thrs=np.array([0.75]), max_dets=self.max_dets)
        f = lambda v: -1.0 if v is None else 100.0 * v  # noqa: E731
        out = {"AP": f(ap), "AP50": f(ap50), "AP75": f(ap75)}
        for name, key in (("small", "APs"), ("medium", "APm"), ("large", "APl")):   # COCOeval.summarize lines 4-6
            out[key] = f(coco_ap(self._gts, self._preds, self.num_classes, max_dets=self.max_dets, area_rng=COCO_AREA_RNG[name]))
        return out


def eval_threshold_set():
    """The one threshold set of the device evaluator: COCO_IOU_THRS together with 0.5 and 0.75, duplicates removed by exact value -- so AP50 / AP75 use the very
    doubles the host evaluator hands to coco_ap.  -> (thresholds, indices of COCO_IOU_THRS in it, index of 0.5, index of 0.75)"""
    thrs: List[float] = []
    for t in [float(t) for t in COCO_IOU_THRS] + [0.5, 0.75]:
        if t not in thrs:
            thrs.append(t)
    return thrs, [thrs.index(float(t)) for t in COCO_IOU_THRS], thrs.index(0.5), thrs.index(0.75)


# the area ranges of one launch: the host evaluator scores AP / AP50 / AP75 with area_rng=None (nothing ignored: an infinite range), then COCO's small / medium / large
EVAL_AREA_RNGS = ((float("-inf"), float("inf")), COCO_AREA_RNG["small"], COCO_AREA_RNG["medium"], COCO_AREA_RNG["large"])


class GpuDetectionEvaluator:
    """DetectionEvaluator with the greedy matching on the MI355X (ops.match_detections -> ymi_eval_match): update() / update_from_slab() launch ONE kernel per batch on
    the current stream for all six numbers (four area ranges x one threshold set) and keep the flags on the device -- no copy to the host, no synchronisation --;
    compute() makes one device-to-host transfer, rebuilds every class's records in the host evaluator's order (update order, image, rank) and runs coco_ap's own
    float64 accumulation (_ap_per_threshold).  The dict equals DetectionEvaluator.compute()'s on the same inputs.  At most 1024 detections and 1024 ground truths per
    image; no CPU fallback."""

    def __init__(self, num_classes: int = 80, max_dets: Optional[int] = COCO_MAX_DETS):
        self.num_classes = num_classes
        self.max_dets = max_dets
        self._thrs, self._ap_idx, self._i50, self._i75 = eval_threshold_set()
        self._batches: List[tuple] = []   # per launch: (tp, ig, rank, scores, labels) on the device
        self._n_gt = None                 # (4, C) int32 on the device, added to by every launch
        self._status = None               # int32[4] on the device, ORed into by every launch
        self._images = 0

    @staticmethod
    def _pad_targets(targets, device):
        """List[Dict{boxes (g,4), labels (g)}] -> (gt_boxes (N,G,4) fp32, gt_labels (N,G) int32, gt_counts (N) int32) on `device`; a 3-tuple of tensors passes through"""
        import torch
        if isinstance(targets, tuple) and len(targets) == 3 and all(hasattr(t, "is_cuda") for t in targets):
            return targets
        n = len(targets)
        lens = [int(len(t["labels"])) for t in targets]
        g = max(lens + [1])
        if all(hasattr(t["boxes"], "is_cuda") and t["boxes"].is_cuda for t in targets) and n:
            gb = torch.zeros(n, g, 4, device=device, dtype=torch.float32)
            gl = torch.zeros(n, g, device=device, dtype=torch.int32)
            for i, t in enumerate(targets):
                if lens[i]:
                    gb[i, : lens[i]] = t["boxes"].detach().to(torch.float32).reshape(-1, 4)
                    gl[i, : lens[i]] = t["labels"].detach().to(torch.int32)
            return gb, gl, torch.tensor(lens, dtype=torch.int32).to(device, non_blocking=True)
        gb = np.zeros((n, g, 4), np.float32)
        gl = np.zeros((n, g), np.int32)
        for i, t in enumerate(targets):
            if lens[i]:
                gb[i, : lens[i]] = DetectionEvaluator._np(t, ("boxes",))["boxes"].reshape(-1, 4)
                gl[i, : lens[i]] = np.asarray(DetectionEvaluator._np(t, ("labels",))["labels"]).astype(np.int64).clip(-(2 ** 31), 2 ** 31 - 1)
        return (torch.from_numpy(gb).to(device, non_blocking=True), torch.from_numpy(gl).to(device, non_blocking=True),
                torch.tensor(lens, dtype=torch.int32).to(device, non_blocking=True))

    def update_from_slab(self, slab, targets) -> None:
        """slab = (boxes (N,K,4), scores (N,K), labels (N,K), counts (N)) of the GLOBAL batch on the device -- what `PendingDetections.gathered()` /
        `dist.all_gather_slab` return; targets: ground truth of the same N images in the same order (List[Dict{boxes, labels}], or the padded device tensors
        (gt_boxes (N,G,4), gt_labels (N,G), gt_counts (N))).  One launch on the current stream; nothing is read back (a stale row or a bad label surfaces in compute())."""
        import torch
        from .. import ops
        boxes, scores, labels, counts = slab
        n = int(scores.shape[0])
        if not isinstance(targets, tuple) and len(targets) != n:
            raise ValueError("one target per prediction is required")
        if n == 0:
            return
        gb, gl, gc = self._pad_targets(targets, boxes.device)
        if self._n_gt is None:
            self._n_gt = torch.zeros(len(EVAL_AREA_RNGS), self.num_classes, device=boxes.device, dtype=torch.int32)
            self._status = torch.zeros(4, device=boxes.device, dtype=torch.int32)
        tp, ig, rank, _, _ = ops._launch_eval_match(boxes, scores, labels, counts, gb, gl, gc, self.num_classes, self._thrs, EVAL_AREA_RNGS, self.max_dets,
                                                    n_gt=self._n_gt, status=self._status)
        # the slab's buffers are the caller's to reuse: keep copies of what compute() needs (device to device, on the same stream)
        self._batches.append((tp, ig, rank, scores.detach().to(torch.float32, copy=True), labels.detach().to(torch.int32, copy=True)))
        self._images += n

    def update(self, preds: Sequence[Dict], targets: Sequence[Dict]) -> None:
        """preds: the model's List[Dict{boxes, scores, labels}] (device tensors); targets: List[Dict{boxes, labels}] (xyxy, same image order): padded into a slab, then
        update_from_slab"""
        import torch
        if len(preds) != len(targets):
            raise ValueError("one target per prediction is required")
        if not preds:
            return
        dev = preds[0]["boxes"].device
        lens = [int(p["scores"].shape[0]) for p in preds]
        k = max(lens + [1])
        boxes = torch.zeros(len(preds), k, 4, device=dev, dtype=torch.float32)
        scores = torch.zeros(len(preds), k, device=dev, dtype=torch.float32)
        labels = torch.zeros(len(preds), k, device=dev, dtype=torch.int64)
        for i, p in enumerate(preds):
            if lens[i]:
                boxes[i, : lens[i]] = p["boxes"].detach().to(torch.float32)
                scores[i, : lens[i]] = p["scores"].detach().to(torch.float32)
                labels[i, : lens[i]] = p["labels"].detach().to(torch.int64)
        self.update_from_slab((boxes, scores, labels, torch.tensor(lens, dtype=torch.int32).to(dev, non_blocking=True)), targets)

    def merge(self, other: "GpuDetectionEvaluator") -> None:
        """fold in another accumulator of the same device (ranks own disjoint image shards); no synchronisation"""
        if other._n_gt is None:
            return
        if self._n_gt is None:
            self._n_gt, self._status = other._n_gt.clone(), other._status.clone()
        else:
            self._n_gt += other._n_gt
            self._status |= other._status
        self._batches += other._batches
        self._images += other._images

    def compute(self) -> Dict[str, float]:
        import torch
        from ..ops import _raise_eval_status
        if not self._images:
            return {"AP": -1.0, "AP50": -1.0, "AP75": -1.0, "APs": -1.0, "APm": -1.0, "APl": -1.0}
        # ONE transfer: every buffer as bytes, concatenated on the device
        parts = [self._status, self._n_gt] + [t for b in self._batches for t in b]
        flat = torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in parts]).cpu().numpy()
        arrays, off = [], 0
        for t in parts:
            nbytes = t.numel() * t.element_size()
            arrays.append(flat[off: off + nbytes].view({torch.int32: np.int32, torch.int16: np.uint16, torch.float32: np.float32}[t.dtype]).reshape(tuple(t.shape)))
            off += nbytes
        _raise_eval_status(int(arrays[0][1]))
        n_gt = arrays[1]
        # every record that takes part, in the host's order within a class: update order, image, rank
        cls, score, tpw, igw = [], [], [], []
        for b in range(len(self._batches)):
            tp, ig, rank, sc, lab = arrays[2 + 5 * b: 7 + 5 * b]
            img, slot = np.nonzero(rank >= 0)
            o = np.lexsort((rank[img, slot], img))
            img, slot = img[o], slot[o]
            cls.append(lab[img, slot]); score.append(sc[img, slot].astype(np.float64)); tpw.append(tp[:, img, slot]); igw.append(ig[:, img, slot])
        cls, score, tpw, igw = np.concatenate(cls), np.concatenate(score), np.concatenate(tpw, 1), np.concatenate(igw, 1)
        o = np.argsort(cls, kind="stable")
        cls, score, tpw, igw = cls[o], score[o], tpw[:, o], igw[:, o]
        first = np.searchsorted(cls, np.arange(self.num_classes + 1), side="left")
        bits = np.arange(len(self._thrs), dtype=np.uint16)
        f = lambda v: -1.0 if v is None else 100.0 * v  # noqa: E731

        def ap(r, idx):
            """coco_ap's outer loop for area range r and the thresholds thrs[idx]"""
            aps = []
            for c in range(self.num_classes):
                if n_gt[r, c] == 0:
                    continue
                lo, hi = first[c], first[c + 1]
                if lo == hi:
                    aps.append(0.0)
                    continue
                tps = ((tpw[r, lo:hi, None] >> bits[idx]) & 1).astype(bool)
                igs = ((igw[r, lo:hi, None] >> bits[idx]) & 1).astype(bool)
                aps.append(float(np.mean(_ap_per_threshold(score[lo:hi], tps, igs, int(n_gt[r, c])))))
            return float(np.mean(aps)) if aps else None

        return {"AP": f(ap(0, self._ap_idx)), "AP50": f(ap(0, [self._i50])), "AP75": f(ap(0, [self._i75])),
                "APs": f(ap(1, self._ap_idx)), "APm": f(ap(2, self._ap_idx)), "APl": f(ap(3, self._ap_idx))}
