"""Op-level Python wrappers over the C ABI (tests, stand-alone API pieces).  No fallbacks."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch
from torch import Tensor

from . import _lib
from ._lib import YmiError, check
from .engine import Plan, View


def batched_nms(boxes: Tensor, scores: Tensor, labels: Tensor, iou_threshold: float) -> Tensor:
    """Class-aware NMS of one image on the MI355X; returns kept indices (int64) in score-descending
    stable order -- the contract of torchvision.ops.batched_nms as called at
    yolort/models/box_head.py:422.  Scores may be any float values: negative ones, signed zeros
    (-0.0 and +0.0 tie, the lower index first), infinities and subnormals are ordered as floats compare.  NaN scores and NaN
    coordinates are outside the contract: what is returned for them is unspecified.  At most 2^20 - 1 boxes per call."""
    lib = _lib.load(require_gpu=True)
    if not boxes.is_cuda:
        raise YmiError("batched_nms runs on an MI355X only (no CPU fallback)")
    n = int(scores.numel())
    dev = boxes.device
    b = boxes.detach().to(torch.float32).contiguous()
    s = scores.detach().to(torch.float32).contiguous()
    # torchvision accepts arbitrary int64 category ids; the kernel's records carry a 12-bit class field.  Only EQUALITY of ids matters to the suppression, so the ids are
    # renumbered densely (sorted unique -> 0 .. u-1) first; more than 4096 distinct classes in one call are refused instead of aliased
    if n > 0:
        uniq, l = torch.unique(labels.detach().reshape(-1), sorted=True, return_inverse=True)
        if uniq.numel() > 4096:
            raise YmiError(f"batched_nms: {uniq.numel()} distinct category ids in one call (the kernel holds 4096)")
        l = l.to(torch.int32).contiguous()
    else:
        l = labels.detach().to(torch.int32).contiguous()
    keep = torch.empty(max(n, 1), device=dev, dtype=torch.int32)
    count = torch.zeros(1, device=dev, dtype=torch.int32)
    ws = torch.empty(lib.ymi_nms_ws_bytes(n), device=dev, dtype=torch.uint8)
    check(lib.ymi_batched_nms(b.data_ptr(), s.data_ptr(), l.data_ptr(), n, float(iou_threshold), keep.data_ptr(), count.data_ptr(),
                              ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "ymi_batched_nms")
    k = int(count.item())
    return keep[:k].to(torch.int64)


def nms(boxes: Tensor, scores: Tensor, iou_threshold: float) -> Tensor:
    """torchvision.ops.nms on the MI355X: greedy suppression over ALL boxes (no classes), IoU > iou_threshold strict, fp32; returns kept indices (int64) in
    score-descending stable order.  The score contract is batched_nms's (any non-NaN float, -0.0 and +0.0 tie, the lower index first); at most 2^20 - 1 boxes per call.
    One workgroup walks the boxes (ymi_nms, include/yolort_amd.h); no CPU fallback."""
    lib = _lib.load(require_gpu=True)
    if not boxes.is_cuda or not scores.is_cuda:
        raise YmiError("nms runs on an MI355X only (no CPU fallback)")
    n = int(scores.numel())
    dev = boxes.device
    b = boxes.detach().to(torch.float32).contiguous()
    s = scores.detach().to(torch.float32).contiguous()
    keep = torch.empty(max(n, 1), device=dev, dtype=torch.int32)
    count = torch.zeros(1, device=dev, dtype=torch.int32)
    ws = torch.empty(lib.ymi_nms_ws_bytes(n), device=dev, dtype=torch.uint8)
    check(lib.ymi_nms(b.data_ptr(), s.data_ptr(), n, float(iou_threshold), keep.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "ymi_nms")
    k = int(count.item())
    return keep[:k].to(torch.int64)


def _launch_eval_match(boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, gt_boxes: Tensor, gt_labels: Tensor, gt_counts: Tensor, num_classes: int,
                       iou_thrs, area_rngs, max_dets, tp: Optional[Tensor] = None, ig: Optional[Tensor] = None, rank: Optional[Tensor] = None,
                       n_gt: Optional[Tensor] = None, status: Optional[Tensor] = None):
    """One ymi_eval_match launch on the current stream, without a synchronisation: -> (tp, ig, rank, n_gt, status).  Output buffers handed in are written in place
    (n_gt is added to, status[1] ORed into: the caller zeroed them once); missing ones are allocated (tp / ig / n_gt / status zeroed, rank filled with -1)."""
    lib = _lib.load(require_gpu=True)
    if not all(t.is_cuda for t in (boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts)):
        raise YmiError("match_detections runs on an MI355X only (no CPU fallback)")
    n, k = int(scores.shape[0]), int(scores.shape[1])
    g = int(gt_labels.shape[1])
    if tuple(boxes.shape) != (n, k, 4) or tuple(labels.shape) != (n, k) or tuple(counts.shape) != (n,):
        raise YmiError(f"match_detections: expected the slab (N,K,4) / (N,K) / (N,K) / (N), got {tuple(boxes.shape)} {tuple(scores.shape)} {tuple(labels.shape)} {tuple(counts.shape)}")
    if tuple(gt_boxes.shape) != (n, g, 4) or tuple(gt_counts.shape) != (n,):
        raise YmiError(f"match_detections: expected ground truth (N,G,4) / (N,G) / (N), got {tuple(gt_boxes.shape)} {tuple(gt_labels.shape)} {tuple(gt_counts.shape)}")
    if iou_thrs is None:
        from .utils.metrics import COCO_IOU_THRS as iou_thrs   # numpy's linspace(.5, .95, 10): the host evaluator's own grid (metrics imports ops lazily too)
    thrs = [float(t) for t in iou_thrs]
    rngs = [(float("-inf"), float("inf"))] if area_rngs is None else [(float(lo), float(hi)) for lo, hi in area_rngs]
    dev = boxes.device
    d = _lib.EvalDesc()
    d.n, d.k, d.g, d.num_thrs, d.num_rngs = n, k, g, len(thrs), len(rngs)
    d.max_dets, d.num_classes = (0 if max_dets is None else int(max_dets)), int(num_classes)
    for i, t in enumerate(thrs[:_lib.EVAL_MAX_THRS]):
        d.thrs[i] = t
    for i, (lo, hi) in enumerate(rngs[:_lib.EVAL_MAX_RNGS]):
        d.area_rng[i][0], d.area_rng[i][1] = lo, hi
    nr = max(min(len(rngs), _lib.EVAL_MAX_RNGS), 1)
    tp = torch.zeros(nr, n, k, device=dev, dtype=torch.int16) if tp is None else tp      # uint16 words (bit t per threshold) in int16 storage
    ig = torch.zeros(nr, n, k, device=dev, dtype=torch.int16) if ig is None else ig
    rank = torch.full((n, k), -1, device=dev, dtype=torch.int32) if rank is None else rank
    n_gt = torch.zeros(nr, max(int(num_classes), 1), device=dev, dtype=torch.int32) if n_gt is None else n_gt
    status = torch.zeros(4, device=dev, dtype=torch.int32) if status is None else status
    ins = [boxes.detach().to(torch.float32).contiguous(), scores.detach().to(torch.float32).contiguous(), labels.detach().to(torch.int64).contiguous(),
           counts.detach().to(torch.int32).contiguous(), gt_boxes.detach().to(torch.float32).contiguous(), gt_labels.detach().to(torch.int32).contiguous(),
           gt_counts.detach().to(torch.int32).contiguous()]
    d.boxes, d.scores, d.labels, d.counts, d.gt_boxes, d.gt_labels, d.gt_counts = [t.data_ptr() for t in ins]
    for t, shape, dt in ((tp, (nr, n, k), torch.int16), (ig, (nr, n, k), torch.int16), (rank, (n, k), torch.int32), (n_gt, (nr, int(num_classes)), torch.int32)):
        if not t.is_cuda or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
            raise YmiError(f"match_detections: an output buffer must be a contiguous device tensor of shape {shape} and dtype {dt}")
    d.tp, d.ig, d.rank, d.n_gt, d.status = tp.data_ptr(), ig.data_ptr(), rank.data_ptr(), n_gt.data_ptr(), status.data_ptr()
    check(lib.ymi_eval_match(C.byref(d), _lib.stream_ptr()), "ymi_eval_match")
    return tp, ig, rank, n_gt, status


def _raise_eval_status(bits: int) -> None:
    if bits & _lib.EVAL_STATUS_STALE_ROW:
        raise ValueError("the slab still holds a stale shard: take PendingDetections.gathered() (it resolves the second round) first")
    if bits & _lib.EVAL_STATUS_BAD_LABEL:
        raise ValueError("a detection or ground-truth label lies outside [0, num_classes)")


def match_detections(boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, gt_boxes: Tensor, gt_labels: Tensor, gt_counts: Tensor, num_classes: int,
                     iou_thrs: Optional[Sequence[float]] = None, area_rngs: Optional[Sequence[Sequence[float]]] = None, max_dets: Optional[int] = None):
    """The greedy matching of the COCO detection protocol on the MI355X (ymi_eval_match, include/yolort_amd.h): the detection slab (boxes (N,K,4), scores (N,K), labels
    (N,K) int64, counts (N)) exactly as `PendingDetections.gathered()` / `dist.all_gather_slab` return it against padded ground truth (gt_boxes (N,G,4), gt_labels (N,G),
    gt_counts (N)) -> (tp, ig, rank, n_gt): tp / ig (R,N,K) int16 holding uint16 words with bit t per IoU threshold, rank (N,K) int32 (the position within the
    (image, class) score order -- descending, ties in slab order, NaN scores last --, -1 = takes no part), n_gt (R,C) int32 non-ignored ground truths per class.  iou_thrs: at most 16 thresholds in (0, 1] (None: COCO's
    0.50:0.05:0.95); area_rngs: at most 4 (lo, hi) pairs (None: one range that ignores nothing); max_dets: per (image, class), None = no cut.  K, G <= 1024.  Exactly the
    flags of yolort_amd.utils.metrics.coco_ap's matching loop.  Raises ValueError for a stale slab row or a label outside [0, num_classes) (this reads the status word:
    one synchronisation; GpuDetectionEvaluator defers it to compute()).  No CPU fallback."""
    tp, ig, rank, n_gt, status = _launch_eval_match(boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts, num_classes, iou_thrs, area_rngs, max_dets)
    _raise_eval_status(int(status[1].item()))
    return tp, ig, rank, n_gt


def val_match(boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, gt_boxes: Tensor, gt_labels: Tensor, gt_counts: Tensor, num_classes: int, *,
              conf: float, thrs: Sequence[float], class_aware: bool, matrix: Optional[Tensor] = None, status: Optional[Tensor] = None, count_all_fp: bool = False):
    """The one-to-one matching by IoU of YOLOv5's val.py on the MI355X (ymi_val_match, include/yolort_amd.h): the detection slab (boxes (N,K,4), scores (N,K), labels
    (N,K) int64, counts (N)) against padded ground truth (gt_boxes (N,G,4), gt_labels (N,G), gt_counts (N)) -> (match (N,K) int32: the matched ground-truth index or
    -1, iou (N,K) fp32: the matched IoU, tp (N,K,T) uint8: matched and IoU >= thrs[t], status int32[4]) on the device.  A detection takes part iff score > conf
    (-inf: all); thrs are at most 10 fp32 thresholds in [0, 1], thrs[0] the admission threshold: class_aware=False admits IoU > thrs[0] between ANY classes (the
    confusion matrix's rule), class_aware=True IoU >= thrs[0] within a class (the rule behind ap_per_class).  Each detection keeps its best admissible ground truth
    (ties: lowest index), each ground truth its best such detection (ties: lowest slot); a displaced detection stays unmatched.  `matrix`: an int32 (C+1, C+1) device
    tensor ADDED to, matrix[pred, true], background last; an unmatched candidate counts as [label, C] only in an image with at least one match (the reference's
    quirk) unless count_all_fp.  `status` (int32[4], zeroed by the caller) is ORed into: status[1] holds _lib.VAL_STATUS_* bits.  K, G <= 1024, C <= 4096.  One launch
    on the current stream, no synchronisation, nothing read back (capturable).  No CPU fallback."""
    lib = _lib.load(require_gpu=True)
    if not all(t.is_cuda for t in (boxes, scores, labels, counts, gt_boxes, gt_labels, gt_counts)):
        raise YmiError("val_match runs on an MI355X only (no CPU fallback)")
    n, k = int(scores.shape[0]), int(scores.shape[1])
    g = int(gt_labels.shape[1])
    if tuple(boxes.shape) != (n, k, 4) or tuple(labels.shape) != (n, k) or tuple(counts.shape) != (n,):
        raise YmiError(f"val_match: expected the slab (N,K,4) / (N,K) / (N,K) / (N), got {tuple(boxes.shape)} {tuple(scores.shape)} {tuple(labels.shape)} {tuple(counts.shape)}")
    if tuple(gt_boxes.shape) != (n, g, 4) or tuple(gt_counts.shape) != (n,):
        raise YmiError(f"val_match: expected ground truth (N,G,4) / (N,G) / (N), got {tuple(gt_boxes.shape)} {tuple(gt_labels.shape)} {tuple(gt_counts.shape)}")
    thrs = [float(t) for t in thrs]
    nc, dev = int(num_classes), boxes.device
    d = _lib.ValDesc()
    d.n, d.k, d.g, d.num_thrs, d.num_classes = n, k, g, len(thrs), nc
    d.class_aware, d.flags, d.conf = int(bool(class_aware)), (_lib.VAL_COUNT_ALL_FP if count_all_fp else 0), float(conf)
    for i, t in enumerate(thrs[:_lib.VAL_MAX_THRS]):
        d.thrs[i] = t
    nt = max(min(len(thrs), _lib.VAL_MAX_THRS), 1)
    match = torch.empty(n, k, device=dev, dtype=torch.int32)
    iou = torch.empty(n, k, device=dev, dtype=torch.float32)
    tp = torch.empty(n, k, nt, device=dev, dtype=torch.uint8)
    status = torch.zeros(4, device=dev, dtype=torch.int32) if status is None else status
    for t, shape, name in ((matrix, (nc + 1, nc + 1), "matrix"), (status, (4,), "status")):
        if t is not None and (not t.is_cuda or tuple(t.shape) != shape or t.dtype != torch.int32 or not t.is_contiguous()):
            raise YmiError(f"val_match: {name} must be a contiguous int32 device tensor of shape {shape}")
    ins = [boxes.detach().to(torch.float32).contiguous(), scores.detach().to(torch.float32).contiguous(), labels.detach().to(torch.int64).contiguous(),
           counts.detach().to(torch.int32).contiguous(), gt_boxes.detach().to(torch.float32).contiguous(), gt_labels.detach().to(torch.int32).contiguous(),
           gt_counts.detach().to(torch.int32).contiguous()]
    d.boxes, d.scores, d.labels, d.counts, d.gt_boxes, d.gt_labels, d.gt_counts = [t.data_ptr() for t in ins]
    d.match, d.iou, d.tp, d.status = match.data_ptr(), iou.data_ptr(), tp.data_ptr(), status.data_ptr()
    d.matrix = matrix.data_ptr() if matrix is not None else None
    check(lib.ymi_val_match(C.byref(d), _lib.stream_ptr()), "ymi_val_match")
    return match, iou, tp, status


def _raise_val_status(bits: int) -> None:
    if bits & _lib.VAL_STATUS_STALE_ROW:
        raise ValueError("the slab still holds a stale shard: take PendingDetections.gathered() (it resolves the second round) first")
    if bits & _lib.VAL_STATUS_BAD_LABEL:
        raise ValueError("a detection or ground-truth label lies outside [0, num_classes)")
    if bits & _lib.VAL_STATUS_BAD_COUNT:
        raise ValueError("a slab count exceeds the slab's K slots")


def nv12_planes(frame):
    """A video frame in NV12 -> (y, uv, h, w): the Y plane (h, w) and the CbCr plane (h / 2, w) as 2-D uint8 views with stride(1) == 1 (the row stride is the pitch).
    `frame` is the packed buffer -- a contiguous 2-D uint8 tensor (3h / 2, w): Y rows, then chroma rows -- or a pair (y, uv) of such views, which is how pitched decoder
    surfaces arrive.  ValueError for anything else; sides are even and >= 2, pitches even, the chroma plane 2-byte aligned."""
    if isinstance(frame, Tensor):
        if frame.dim() != 2 or frame.dtype != torch.uint8 or not frame.is_contiguous() or frame.shape[0] % 3 != 0:
            raise ValueError(f"an NV12 frame is a contiguous 2-D uint8 tensor (3h/2, w) or a pair (y, uv), got {frame.dtype} {tuple(frame.shape)}")
        h = frame.shape[0] // 3 * 2
        y, uv = frame[:h], frame[h:]
    else:
        if len(frame) != 2 or not all(isinstance(t, Tensor) and t.dim() == 2 and t.dtype == torch.uint8 for t in frame):
            raise ValueError("an NV12 frame is a contiguous 2-D uint8 tensor (3h/2, w) or a pair (y, uv) of 2-D uint8 tensors")
        y, uv = frame
    h, w = int(y.shape[0]), int(y.shape[1])
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f"NV12 frames have even sides >= 2, got {h} x {w}")
    if tuple(uv.shape) != (h // 2, w):
        raise ValueError(f"the CbCr plane of a {h} x {w} frame is ({h // 2}, {w}) bytes, got {tuple(uv.shape)}")
    for t, name in ((y, "Y"), (uv, "CbCr")):
        if t.stride(1) != 1 or t.stride(0) < w or t.stride(0) % 2:
            raise ValueError(f"the {name} plane needs stride(1) == 1 and an even row pitch >= the width, got strides {tuple(t.stride())}")
    if uv.data_ptr() % 2:
        raise ValueError("the CbCr plane must be 2-byte aligned")
    if y.device != uv.device:
        raise ValueError("the planes of a frame live on one device")
    return y, uv, h, w


def _nv12_params(matrix: str, full_range: bool):
    if matrix not in _lib.NV12_MATRIX:
        raise ValueError(f"matrix must be 'bt601' or 'bt709', got {matrix!r}")
    return _lib.NV12_MATRIX[matrix], _lib.NV12_FULL if full_range else _lib.NV12_LIMITED


def nv12_to_rgb(frame, *, matrix: str = "bt601", full_range: bool = False) -> Tensor:
    """One NV12 frame (see nv12_planes) -> interleaved RGB (h, w, 3) uint8 on the MI355X (ymi_nv12_to_rgb): the integer conversion contract of include/yolort_amd.h
    -- nearest chroma, BT.601 / BT.709, limited / full range, coefficients in 2^-14 units -- exactly reproducible.  The image `YOLOv5.forward`, ops.crop_detections and
    ops.draw_detections take for video frames.  No CPU fallback."""
    lib = _lib.load(require_gpu=True)
    y, uv, h, w = nv12_planes(frame)
    m, r = _nv12_params(matrix, full_range)
    if not y.is_cuda:
        raise YmiError("nv12_to_rgb runs on an MI355X only (no CPU fallback)")
    rgb = torch.empty((h, w, 3), device=y.device, dtype=torch.uint8)
    check(lib.ymi_nv12_to_rgb(y.data_ptr(), uv.data_ptr(), y.stride(0), uv.stride(0), h, w, m, r, rgb.data_ptr(), _lib.stream_ptr()), "ymi_nv12_to_rgb")
    return rgb


def launch_letterbox_nv12(planes, sizes, pads, out_ptr, hb: int, wb: int, c_out: int, out_dtype: torch.dtype, matrix: int, rng: int, fill: float, stream=None) -> None:
    """one ymi_letterbox_nv12 call on `stream` for frames already taken apart by nv12_planes: planes = [(y, uv, h, w)], sizes = [(h_res, w_res)], pads = [(top, left)]"""
    lib = _lib.load(require_gpu=True)
    n = len(planes)
    d = _lib.Nv12Desc()
    ys = (C.c_void_p * max(n, 1))(*[p[0].data_ptr() for p in planes])
    uvs = (C.c_void_p * max(n, 1))(*[p[1].data_ptr() for p in planes])
    pitch = (C.c_int32 * max(2 * n, 1))(*[v for p in planes for v in (p[0].stride(0), p[1].stride(0))])
    geom = (C.c_int32 * max(6 * n, 1))(*[v for p, s_, q in zip(planes, sizes, pads) for v in (p[2], p[3], s_[0], s_[1], q[0], q[1])])
    d.y, d.uv = C.cast(ys, C.POINTER(C.c_void_p)), C.cast(uvs, C.POINTER(C.c_void_p))
    d.pitch, d.geom = C.cast(pitch, C.POINTER(C.c_int32)), C.cast(geom, C.POINTER(C.c_int32))
    d.n, d.matrix, d.range, d.out = n, matrix, rng, out_ptr
    d.hb, d.wb, d.c_out, d.out_dtype, d.fill = hb, wb, c_out, _lib.dtype_code(out_dtype), float(fill)
    check(lib.ymi_letterbox_nv12(C.byref(d), _lib.stream_ptr(stream)), "ymi_letterbox_nv12")


def letterbox_nv12(frames, sizes, pads, canvas_hw, *, matrix: str = "bt601", full_range: bool = False, dtype: torch.dtype = torch.float16, c_out: int = 4,
                   fill: float = 114 / 255) -> Tensor:
    """NV12 frames (see nv12_planes) letterboxed onto one canvas in ONE launch per 64 frames, the colour conversion fused into the letterbox kernel
    (ymi_letterbox_nv12) -> (n, hb, wb, c_out) of `dtype` (fp16 / bf16 / fp32): bit for bit the canvas ymi_letterbox writes for nv12_to_rgb's images.  sizes =
    [(h_res, w_res)] and pads = [(top, left)] per frame, as YOLOTransform.geometry returns them; channels 3 and above are zero.  No CPU fallback."""
    planes = [nv12_planes(f) for f in frames]
    m, r = _nv12_params(matrix, full_range)
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"letterbox_nv12: dtype must be float16, bfloat16 or float32, got {dtype}")
    if len(sizes) != len(planes) or len(pads) != len(planes):
        raise ValueError(f"letterbox_nv12: {len(planes)} frames, {len(sizes)} sizes, {len(pads)} pads")
    if not planes:
        raise ValueError("letterbox_nv12: no frames")
    if not all(p[0].is_cuda for p in planes):
        raise YmiError("letterbox_nv12 runs on an MI355X only (no CPU fallback)")
    hb, wb = int(canvas_hw[0]), int(canvas_hw[1])
    out = torch.empty((len(planes), hb, wb, int(c_out)), device=planes[0][0].device, dtype=dtype)
    launch_letterbox_nv12(planes, sizes, pads, out.data_ptr(), hb, wb, int(c_out), dtype, m, r, fill)
    return out


def crop_detections(images: Sequence[Tensor], boxes: Tensor, counts: Tensor, size, *, gain: float = 1.02, pad: float = 10, square: bool = False,
                    mean: Optional[Sequence[float]] = None, std: Optional[Sequence[float]] = None, dtype: torch.dtype = torch.float16, capacity: Optional[int] = None):
    """Every detection of the slab cut out of its original image and resized to `size` = (out_h, out_w), on the MI355X in one launch per batch (ymi_crop_resize,
    include/yolort_amd.h): the device form of the reference's `Detections.crop()` / save_one_box (yolort/v5/utils/plots.py:545-558) and of apply_classifier's cut-outs
    (yolort/v5/utils/general.py:691-723).  images: the list `YOLOv5.forward` takes -- (3, h, w) float in [0, 1] or uint8, or interleaved (h, w, 3) uint8, one dtype and
    layout per batch, sizes may differ; boxes (n, K, 4) xyxy in original-image coordinates and counts (n,): the slab form.  -> (crops, index, total), device tensors of
    full capacity and NO synchronisation: crops (capacity, 3, out_h, out_w) of `dtype` (fp16 / bf16 / fp32), image-major in the slab's order; index (capacity, 6) int32
    rows {image, detection, x1, y1, x2, y2} (the integer rectangle that was cut); total int32[2] = {crops written, status bits _lib.CROP_STATUS_CAPACITY /
    _lib.CROP_STATUS_BAD_COUNT}.  Rows at or beyond total[0] are uninitialised.  capacity defaults to n * K.
    The rectangle is save_one_box's, in its fp32 order: box -> centre and size, (square: both sides the larger one), side * gain + pad, corners truncated toward zero
    and clipped to the image; an empty rectangle gives an all-zero crop that keeps its row (its index row holds the clipped corners), a non-finite box likewise with the rectangle (0, 0, 0, 0).  The defaults are save_one_box's; apply_classifier's
    recipe is square=True, gain=1.3, pad=30, size=(224, 224) -- but the reference pads in CANVAS pixels before scale_coords while this op pads in image pixels, so that
    recipe is not claimed as parity.  The resize is F.interpolate(mode="bilinear", align_corners=False) of the cut-out (bit for bit where the weights are powers of
    two, a few fp32 ulps elsewhere), optionally followed by (v - mean[c]) / std[c]; cv2.resize on uint8 uses fixed-point weights and differs in the last bit of a byte."""
    from .models.transform import YOLOTransform
    lib = _lib.load(require_gpu=True)
    images = [images[i] for i in range(len(images))]
    n = len(images)
    if not boxes.is_cuda or not counts.is_cuda or not all(im.is_cuda for im in images):
        raise YmiError("crop_detections runs on an MI355X only (no CPU fallback)")
    if boxes.dim() != 3 or boxes.shape[0] != n or boxes.shape[2] != 4 or tuple(counts.shape) != (n,):
        raise YmiError(f"crop_detections: expected the slab (n, K, 4) / (n,) for {n} images, got {tuple(boxes.shape)} {tuple(counts.shape)}")
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise YmiError(f"crop_detections: dtype must be float16, bfloat16 or float32, got {dtype}")
    if (mean is None) != (std is None):
        raise ValueError("crop_detections: mean and std go together")
    out_h, out_w = int(size[0]), int(size[1])
    k = int(boxes.shape[1])
    cap = n * k if capacity is None else int(capacity)
    hwc = False
    if n:
        kinds = {(im.dtype, YOLOTransform.is_hwc(im)) for im in images}
        if len(kinds) != 1:
            raise YmiError("all images of a batch must share one dtype and layout")
        hwc = YOLOTransform.is_hwc(images[0])
        for im in images:
            if im.dim() != 3 or (im.shape[0] != 3 and not hwc):
                raise ValueError(f"images are expected to be (3, H, W) tensors (or (H, W, 3) uint8), got {tuple(im.shape)}")
        images = [im if im.is_contiguous() else im.contiguous() for im in images]
    dev = boxes.device
    d = _lib.CropDesc()
    ptrs = (C.c_void_p * max(n, 1))(*[im.data_ptr() for im in images])
    hw = (C.c_int32 * max(2 * n, 1))(*[v for im in images for v in YOLOTransform.image_hw(im)])
    b = boxes.detach().to(torch.float32).contiguous()
    c = counts.detach().to(torch.int32).contiguous()
    crops = torch.empty((max(cap, 0), 3, max(out_h, 0), max(out_w, 0)), device=dev, dtype=dtype)
    index = torch.empty((max(cap, 0), 6), device=dev, dtype=torch.int32)
    total = torch.empty(2, device=dev, dtype=torch.int32)
    d.imgs, d.hw = C.cast(ptrs, C.POINTER(C.c_void_p)), C.cast(hw, C.POINTER(C.c_int32))
    d.boxes, d.counts, d.crops, d.index, d.total = b.data_ptr(), c.data_ptr(), crops.data_ptr(), index.data_ptr(), total.data_ptr()
    d.gain, d.pad, d.square, d.normalize = float(gain), float(pad), 1 if square else 0, 0 if mean is None else 1
    if mean is not None:
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("crop_detections: mean and std have one value per channel")
        for i in range(3):
            d.mean[i], d.std[i] = float(mean[i]), float(std[i])
    d.n, d.k, d.cap, d.out_h, d.out_w = n, k, cap, out_h, out_w
    d.in_dtype = _lib.YMI_U8_HWC if hwc else (_lib.dtype_code(images[0].dtype) if n else _lib.YMI_F32)
    d.out_dtype = _lib.dtype_code(dtype)
    check(lib.ymi_crop_resize(C.byref(d), _lib.stream_ptr()), "ymi_crop_resize")
    return crops, index, total


def _nv12_tables(planes):
    """the host arrays every NV12 descriptor takes: plane pointers, n x {pitch_y, pitch_uv}, n x {h, w}"""
    n = len(planes)
    ys = (C.c_void_p * max(n, 1))(*[p[0].data_ptr() for p in planes])
    uvs = (C.c_void_p * max(n, 1))(*[p[1].data_ptr() for p in planes])
    pitch = (C.c_int32 * max(2 * n, 1))(*[v for p in planes for v in (p[0].stride(0), p[1].stride(0))])
    hw = (C.c_int32 * max(2 * n, 1))(*[v for p in planes for v in (p[2], p[3])])
    return ys, uvs, pitch, hw


def crop_detections_nv12(frames, boxes: Tensor, counts: Tensor, size, *, matrix: str = "bt601", full_range: bool = False, gain: float = 1.02, pad: float = 10,
                         square: bool = False, mean: Optional[Sequence[float]] = None, std: Optional[Sequence[float]] = None, dtype: torch.dtype = torch.float16,
                         capacity: Optional[int] = None):
    """crop_detections for NV12 video frames (see nv12_planes: packed (3h/2, w) buffers or (y, uv) pairs of pitched planes), in one launch per batch
    (ymi_crop_resize_nv12): the taps are fetched from the planes and converted on the fly (`matrix` "bt601" / "bt709", limited or full range), so no RGB copy of a
    frame is made.  -> (crops, index, total), BIT FOR BIT crop_detections([nv12_to_rgb(f) for f in frames], ...) with the same keyword arguments.  No
    synchronisation, no CPU fallback."""
    lib = _lib.load(require_gpu=True)
    planes = [nv12_planes(frames[i]) for i in range(len(frames))]
    n = len(planes)
    m, r = _nv12_params(matrix, full_range)
    if not boxes.is_cuda or not counts.is_cuda or not all(p[0].is_cuda for p in planes):
        raise YmiError("crop_detections_nv12 runs on an MI355X only (no CPU fallback)")
    if boxes.dim() != 3 or boxes.shape[0] != n or boxes.shape[2] != 4 or tuple(counts.shape) != (n,):
        raise YmiError(f"crop_detections_nv12: expected the slab (n, K, 4) / (n,) for {n} frames, got {tuple(boxes.shape)} {tuple(counts.shape)}")
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise YmiError(f"crop_detections_nv12: dtype must be float16, bfloat16 or float32, got {dtype}")
    if (mean is None) != (std is None):
        raise ValueError("crop_detections_nv12: mean and std go together")
    out_h, out_w = int(size[0]), int(size[1])
    k = int(boxes.shape[1])
    cap = n * k if capacity is None else int(capacity)
    dev = boxes.device
    d = _lib.CropNv12Desc()
    ys, uvs, pitch, hw = _nv12_tables(planes)
    b = boxes.detach().to(torch.float32).contiguous()
    c = counts.detach().to(torch.int32).contiguous()
    crops = torch.empty((max(cap, 0), 3, max(out_h, 0), max(out_w, 0)), device=dev, dtype=dtype)
    index = torch.empty((max(cap, 0), 6), device=dev, dtype=torch.int32)
    total = torch.empty(2, device=dev, dtype=torch.int32)
    d.y, d.uv = C.cast(ys, C.POINTER(C.c_void_p)), C.cast(uvs, C.POINTER(C.c_void_p))
    d.pitch, d.hw = C.cast(pitch, C.POINTER(C.c_int32)), C.cast(hw, C.POINTER(C.c_int32))
    d.boxes, d.counts, d.crops, d.index, d.total = b.data_ptr(), c.data_ptr(), crops.data_ptr(), index.data_ptr(), total.data_ptr()
    d.gain, d.pad, d.square, d.normalize = float(gain), float(pad), 1 if square else 0, 0 if mean is None else 1
    if mean is not None:
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("crop_detections_nv12: mean and std have one value per channel")
        for i in range(3):
            d.mean[i], d.std[i] = float(mean[i]), float(std[i])
    d.n, d.k, d.cap, d.out_h, d.out_w = n, k, cap, out_h, out_w
    d.matrix, d.range, d.out_dtype = m, r, _lib.dtype_code(dtype)
    check(lib.ymi_crop_resize_nv12(C.byref(d), _lib.stream_ptr()), "ymi_crop_resize_nv12")
    return crops, index, total


# The default colours of draw_detections, the project's own: 20 hues in steps of 7 / 20 of the colour circle (neighbouring classes far apart), saturation 0.85 / 0.6
# and value 1.0 / 0.8 alternating -- RGB.  A detection of class c has DEFAULT_COLORS[c % 20].
DEFAULT_COLORS = ((255, 38, 38), (102, 255, 117), (65, 31, 204), (204, 118, 82), (38, 255, 125), (178, 102, 255), (204, 135, 31), (82, 204, 167), (212, 38, 255), (255, 240, 102),
                  (31, 204, 204), (204, 82, 192), (212, 255, 38), (102, 209, 255), (204, 31, 135), (143, 204, 82), (38, 125, 255), (255, 102, 148), (65, 204, 31), (82, 94, 204))
_render_tables: Dict[tuple, Tensor] = {}   # (kind, content, device) -> device table: built once per names tuple / palette and device


def render_name_table(names: Sequence[str]) -> Tensor:
    """(len(names), 28) uint8 on the host, ymi_render's name table: a length byte, then the ASCII bytes (a character outside ASCII becomes '?'); at most 27 bytes a name"""
    rows = torch.zeros((len(names), _lib.RENDER_NAME_STRIDE), dtype=torch.uint8)
    for i, name in enumerate(names):
        raw = str(name).encode("ascii", "replace")
        if len(raw) > _lib.RENDER_NAME_STRIDE - 1:
            raise ValueError(f"draw_detections: the name of class {i} has {len(raw)} bytes (at most {_lib.RENDER_NAME_STRIDE - 1})")
        rows[i, 0] = len(raw)
        rows[i, 1: 1 + len(raw)] = torch.tensor(list(raw), dtype=torch.uint8)
    return rows


def _render_table(kind: str, content: tuple, dev: torch.device) -> Tensor:
    key = (kind, content, str(dev))
    t = _render_tables.get(key)
    if t is None:
        host = render_name_table(content) if kind == "names" else torch.tensor(content, dtype=torch.uint8).reshape(-1, 3)
        t = _render_tables[key] = host.to(dev)
    return t


def render_defaults(h: int, w: int):
    """(lw, fs) the reference gives an h x w image: Annotator's line width max(round(sum(im.shape) / 2 * 0.003), 2) on an (h, w, 3) array and its PIL branch's font
    size max(round(sum(im.size) / 2 * 0.035), 12) in units of the 11-pixel cell (yolort/v5/utils/plots.py:98-117)"""
    return max(round((h + w + 3) / 2 * 0.003), 2), max(1, round(max(round((h + w) / 2 * 0.035), 12) / 11))


def draw_detections(images: Sequence[Tensor], boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, *, names: Optional[Sequence[str]] = None,
                    colors: Optional[Sequence[Sequence[int]]] = None, line_width=None, font_scale=None, labels_on: bool = True, conf: bool = True,
                    txt_color: Sequence[int] = (255, 255, 255), inplace: bool = False):
    """Every detection of the slab drawn into its original image -- outline, label background, label text -- on the MI355X in one launch per batch (ymi_render,
    include/yolort_amd.h, where the drawing rule is written out): the device form of the reference's `Detections.render()` (yolort/v5/models/common.py:575-652), a host
    loop of one `Annotator.box_label` (yolort/v5/utils/plots.py:98-159) per box.  images: the list `YOLOv5.forward` takes -- (3, h, w) float in [0, 1] or uint8, or
    interleaved (h, w, 3) uint8, one dtype and layout per batch, sizes may differ; boxes (n, K, 4) xyxy in original-image coordinates, scores (n, K), labels (n, K),
    counts (n,): the slab form, K <= 1024.  -> (images, status): the annotated images (the inputs themselves with inplace=True -- they must be contiguous --, clones
    otherwise; the kernel always draws in place) and the int32 status word on the device (_lib.RENDER_STATUS_BAD_COUNT / _STALE_ROW / _BAD_LABEL).  NO synchronisation.
    names: the class names (ASCII, at most 27 bytes each; None draws the class index); colors: (m, 3) RGB rows, class c has colors[c % m] (None: DEFAULT_COLORS);
    line_width / font_scale: one int or one per image (None: the reference's defaults for the image's size, `render_defaults`); font_scale is the integer magnification
    of the 6 x 11 cell; labels_on=False draws outlines only, conf=False leaves the score out.  The outline is PIL's `ImageDraw.rectangle(width=lw)` wherever
    2 * lw <= min(box side) + 1; the text is Pillow's built-in bitmap font cell by cell and has no parity with the reference (it needs a downloaded Arial.ttf or cv2)."""
    from .models.transform import YOLOTransform
    lib = _lib.load(require_gpu=True)
    images = [images[i] for i in range(len(images))]
    n = len(images)
    if not all(t.is_cuda for t in (boxes, scores, labels, counts)) or not all(im.is_cuda for im in images):
        raise YmiError("draw_detections runs on an MI355X only (no CPU fallback)")
    if boxes.dim() != 3 or boxes.shape[0] != n or boxes.shape[2] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2]) or tuple(labels.shape) != tuple(boxes.shape[:2]) or tuple(counts.shape) != (n,):
        raise YmiError(f"draw_detections: expected the slab (n, K, 4) / (n, K) / (n, K) / (n,) for {n} images, got {tuple(boxes.shape)} {tuple(scores.shape)} {tuple(labels.shape)} {tuple(counts.shape)}")
    k = int(boxes.shape[1])
    dev = boxes.device
    hwc = False
    if n:
        kinds = {(im.dtype, YOLOTransform.is_hwc(im)) for im in images}
        if len(kinds) != 1:
            raise YmiError("all images of a batch must share one dtype and layout")
        hwc = YOLOTransform.is_hwc(images[0])
        for im in images:
            if im.dim() != 3 or (im.shape[0] != 3 and not hwc):
                raise ValueError(f"images are expected to be (3, H, W) tensors (or (H, W, 3) uint8), got {tuple(im.shape)}")
        if inplace:
            if not all(im.is_contiguous() for im in images):
                raise YmiError("draw_detections: inplace=True needs contiguous images")
        else:
            images = [im.clone(memory_format=torch.contiguous_format) for im in images]
    sizes = [YOLOTransform.image_hw(im) for im in images]

    def per_image(value, which):
        if value is None:
            return [render_defaults(int(h), int(w))[which] for h, w in sizes]
        return [int(v) for v in value] if isinstance(value, (list, tuple)) else [int(value)] * n

    lws, fss = per_image(line_width, 0), per_image(font_scale, 1)
    if len(lws) != n or len(fss) != n:
        raise ValueError("draw_detections: line_width / font_scale are one value or one per image")
    d = _lib.RenderDesc()
    ptrs = (C.c_void_p * max(n, 1))(*[im.data_ptr() for im in images])
    hw = (C.c_int32 * max(2 * n, 1))(*[int(v) for s in sizes for v in s])
    lw_a, fs_a = (C.c_int32 * max(n, 1))(*lws), (C.c_int32 * max(n, 1))(*fss)
    b = boxes.detach().to(torch.float32).contiguous()
    s = scores.detach().to(torch.float32).contiguous()
    lab = labels.detach().to(torch.int64).contiguous()
    c = counts.detach().to(torch.int32).contiguous()
    table = _render_table("names", tuple(str(v) for v in names), dev) if names is not None else None
    palette = _render_table("colors", tuple(int(v) for row in (DEFAULT_COLORS if colors is None else colors) for v in row), dev)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    d.imgs, d.hw = C.cast(ptrs, C.POINTER(C.c_void_p)), C.cast(hw, C.POINTER(C.c_int32))
    d.lw, d.fs = C.cast(lw_a, C.POINTER(C.c_int32)), C.cast(fs_a, C.POINTER(C.c_int32))
    d.boxes, d.scores, d.labels, d.counts, d.status = b.data_ptr(), s.data_ptr(), lab.data_ptr(), c.data_ptr(), status.data_ptr()
    d.names, d.colors, d.m = (table.data_ptr() if table is not None else None), palette.data_ptr(), int(palette.shape[0])
    for i in range(3):
        d.txt_color[i] = int(txt_color[i])
    d.num_classes = int(table.shape[0]) if table is not None else 2 ** 31 - 1
    d.in_dtype = _lib.YMI_U8_HWC if hwc else (_lib.dtype_code(images[0].dtype) if n else _lib.YMI_F32)
    d.draw_labels, d.draw_conf, d.n, d.k = int(bool(labels_on)), int(bool(conf)), n, k
    check(lib.ymi_render(C.byref(d), _lib.stream_ptr()), "ymi_render")
    return images, status


def draw_detections_nv12(frames, boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, *, matrix: str = "bt601", full_range: bool = False,
                         names: Optional[Sequence[str]] = None, colors: Optional[Sequence[Sequence[int]]] = None, line_width=None, font_scale=None, labels_on: bool = True,
                         conf: bool = True, txt_color: Sequence[int] = (255, 255, 255), inplace: bool = False):
    """draw_detections for NV12 video frames (see nv12_planes: packed (3h/2, w) buffers or (y, uv) pairs of pitched planes): every detection of the slab drawn
    straight into the Y and CbCr planes, the form a hardware encoder takes, in one launch per batch (ymi_render_nv12, include/yolort_amd.h).  Which detection decides a
    luma pixel, and whether as outline, label background or glyph, is draw_detections's rule unchanged (the text has no parity with the reference either); the pixel
    gets the Y of its RGB colour under the integer RGB -> YCbCr contract of the header (`matrix` "bt601" / "bt709", limited or full range), and a chroma pair one of
    whose four luma pixels is decided gets the (Cb, Cr) of the first decided one in raster order.  Nothing else is written: untouched pixels, pairs, pitch padding and
    tiles keep the decoder's bytes.  -> (frames, status): with inplace=True the inputs themselves; otherwise copies -- a packed frame as its clone, a (y, uv) pair as ONE
    packed contiguous (3h/2, w) frame.  The other keyword arguments, the defaults (`render_defaults(h, w)`), K <= 1024 and the status bits are draw_detections's.
    NO synchronisation, no CPU fallback."""
    lib = _lib.load(require_gpu=True)
    frames = [frames[i] for i in range(len(frames))]
    n = len(frames)
    planes = [nv12_planes(f) for f in frames]
    mat, rng = _nv12_params(matrix, full_range)
    if not all(t.is_cuda for t in (boxes, scores, labels, counts)) or not all(p[0].is_cuda for p in planes):
        raise YmiError("draw_detections_nv12 runs on an MI355X only (no CPU fallback)")
    if boxes.dim() != 3 or boxes.shape[0] != n or boxes.shape[2] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2]) or tuple(labels.shape) != tuple(boxes.shape[:2]) or tuple(counts.shape) != (n,):
        raise YmiError(f"draw_detections_nv12: expected the slab (n, K, 4) / (n, K) / (n, K) / (n,) for {n} frames, got {tuple(boxes.shape)} {tuple(scores.shape)} {tuple(labels.shape)} {tuple(counts.shape)}")
    if not inplace:
        frames = [torch.cat([p[0], p[1]]) for p in planes]   # packed and contiguous, whatever came in
        planes = [nv12_planes(f) for f in frames]
    k = int(boxes.shape[1])
    dev = boxes.device

    def per_image(value, which):
        if value is None:
            return [render_defaults(p[2], p[3])[which] for p in planes]
        return [int(v) for v in value] if isinstance(value, (list, tuple)) else [int(value)] * n

    lws, fss = per_image(line_width, 0), per_image(font_scale, 1)
    if len(lws) != n or len(fss) != n:
        raise ValueError("draw_detections_nv12: line_width / font_scale are one value or one per frame")
    d = _lib.RenderNv12Desc()
    ys, uvs, pitch, hw = _nv12_tables(planes)
    lw_a, fs_a = (C.c_int32 * max(n, 1))(*lws), (C.c_int32 * max(n, 1))(*fss)
    b = boxes.detach().to(torch.float32).contiguous()
    s = scores.detach().to(torch.float32).contiguous()
    lab = labels.detach().to(torch.int64).contiguous()
    c = counts.detach().to(torch.int32).contiguous()
    table = _render_table("names", tuple(str(v) for v in names), dev) if names is not None else None
    palette = _render_table("colors", tuple(int(v) for row in (DEFAULT_COLORS if colors is None else colors) for v in row), dev)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    d.y, d.uv = C.cast(ys, C.POINTER(C.c_void_p)), C.cast(uvs, C.POINTER(C.c_void_p))
    d.pitch, d.hw = C.cast(pitch, C.POINTER(C.c_int32)), C.cast(hw, C.POINTER(C.c_int32))
    d.lw, d.fs = C.cast(lw_a, C.POINTER(C.c_int32)), C.cast(fs_a, C.POINTER(C.c_int32))
    d.boxes, d.scores, d.labels, d.counts, d.status = b.data_ptr(), s.data_ptr(), lab.data_ptr(), c.data_ptr(), status.data_ptr()
    d.names, d.colors, d.m = (table.data_ptr() if table is not None else None), palette.data_ptr(), int(palette.shape[0])
    for i in range(3):
        d.txt_color[i] = int(txt_color[i])
    d.num_classes = int(table.shape[0]) if table is not None else 2 ** 31 - 1
    d.matrix, d.range = mat, rng
    d.draw_labels, d.draw_conf, d.n, d.k = int(bool(labels_on)), int(bool(conf)), n, k
    check(lib.ymi_render_nv12(C.byref(d), _lib.stream_ptr()), "ymi_render_nv12")
    return frames, status


def slab_to_list(boxes: Tensor, scores: Tensor, labels: Tensor, counts: Sequence[int]) -> List[Dict[str, Tensor]]:
    """Fixed (N,K,..) slab -> the reference's List[Dict] with keys in its order (box_head.py:427)."""
    out = []
    for i, k in enumerate(counts):
        out.append({"scores": scores[i, :k], "labels": labels[i, :k], "boxes": boxes[i, :k]})
    return out


def postprocess_logits(head_outputs: Sequence[Tensor], strides: Sequence[float], anchors: Sequence[Sequence[float]], num_classes: int,
                       score_thresh: float, nms_thresh: float, detections_per_img: int, cand_cap: Optional[int] = None, multi_label: bool = True, agnostic: bool = False,
                       classes: Optional[Sequence[int]] = None, merge: bool = False, merge_redundant: bool = True) -> List[Dict[str, Tensor]]:
    """Runs the fused post-process on reference-layout head outputs [(N,A,H,W,K)] (A == 3).  multi_label=False: one label per anchor, its best class
    (include/yolort_amd.h YMI_POST_BEST_CLASS).  agnostic=True: one NMS over all boxes of an image, whatever their label (YMI_POST_AGNOSTIC).  classes=[...]: only candidates of these classes, filtered
    before NMS and top-k (YMI_POST_CLASS_FILTER; multi_label=False: an anchor whose best class is not in the set yields nothing); None = no filter.  merge=True: merge-NMS (YMI_POST_MERGE) -- in an image of
    1 < n < 3000 candidates every kept box becomes the score-weighted mean of the candidates of its class (any class with agnostic) whose IoU with it is above nms_thresh, and
    a box with no contributor but itself is dropped unless merge_redundant=False (YMI_POST_MERGE_KEEP_SINGLE)."""
    classes = _lib.normalize_classes(classes, num_classes)
    _lib.load(require_gpu=True)
    h0 = head_outputs[0]
    if not h0.is_cuda:
        raise YmiError("postprocess runs on an MI355X only (no CPU fallback)")
    n = h0.shape[0]
    k = num_classes + 5
    plan_inputs = []
    for ho in head_outputs:
        if ho.shape[1] != 3 or ho.shape[-1] != k:
            raise YmiError(f"expected (N,3,H,W,{k}) head outputs, got {tuple(ho.shape)}")
        cs = (3 * k + 3) // 4 * 4
        nhwc = torch.zeros(n, ho.shape[2], ho.shape[3], cs, device=ho.device, dtype=torch.float32)
        nhwc[..., : 3 * k] = ho.to(torch.float32).permute(0, 2, 3, 1, 4).reshape(n, ho.shape[2], ho.shape[3], 3 * k)
        plan_inputs.append(nhwc)
    cap = cand_cap or max(4096, 2048 * n)
    flags = (0 if multi_label else _lib.POST_BEST_CLASS) | (_lib.POST_AGNOSTIC if agnostic else 0) | _lib.merge_flags(merge, merge_redundant)
    while True:
        plan = Plan(h0.device, torch.float16)
        views = [View(t.view(-1), 0, n, t.shape[1], t.shape[2], 3 * k, t.shape[3]) for t in plan_inputs]
        pb = plan.postprocess(views, strides, anchors, num_classes, score_thresh, nms_thresh, detections_per_img, cap, flags=flags, classes=classes)
        plan.run()
        st = pb.status.cpu().tolist()
        if st[1] == 0:
            break
        if not st[1] & 1:   # YMI_STATUS_PREFIX_SHORT only: the score prefix of a crowded image was too short, take everything
            flags |= _lib.POST_EXACT_FULL
            continue
        need = max(st[0], st[3] * n)     # st[3]: largest per-image count when the per-image sort path overflowed
        cap = max(int(need * 1.25) + 1024, 2 * cap)  # nothing is truncated silently: grow and redo
        cap = n * (1 << ((cap + n - 1) // n - 1).bit_length())   # per-image regions are powers of two
    counts = pb.count.cpu().tolist()
    return slab_to_list(pb.boxes, pb.scores, pb.labels, counts)


def scale_image(x: Tensor, ratio: float, flip: bool = False, gs: int = 32) -> Tensor:
    """A view of augmented inference: (n, 3, h, w) -> (n, 3, H', W'), `x` mirrored left-right first when `flip`, resized by `ratio` with F.interpolate's bilinear
    arithmetic (align_corners=False) and padded with 0.447 to the next multiples of `gs` -- scale_img of yolort/v5/utils/torch_utils.py:288-300 plus the x.flip(3) of
    yolort/v5/models/yolo.py:158, as one kernel over the NHWC4 canvas (ymi_scale_view).  fp16 / bf16 / fp32; ratio 1.0 returns a copy (mirrored when `flip`:
    every bilinear weight is then exactly 1)."""
    lib = _lib.load(require_gpu=True)
    if not x.is_cuda or x.dim() != 4 or x.shape[1] != 3:
        raise YmiError("scale_image takes an (n, 3, h, w) tensor on an MI355X (no CPU fallback)")
    if not 0.0 < ratio <= 1.0:
        raise ValueError(f"scale_image: ratio {ratio} outside (0, 1]")
    n, _, h, w = x.shape
    dt = _lib.dtype_code(x.dtype)
    (sh, sw), (dh, dw) = _lib.tta_view_size(h, w, ratio, gs)
    if sh < 1 or sw < 1:
        raise ValueError(f"scale_image: {h} x {w} at ratio {ratio} leaves no pixel")
    src = torch.zeros(n, h, w, 4, device=x.device, dtype=x.dtype)
    src[..., :3] = x.permute(0, 2, 3, 1)
    dst = torch.empty(n, dh, dw, 4, device=x.device, dtype=x.dtype)
    check(lib.ymi_scale_view(src.data_ptr(), n, h, w, dst.data_ptr(), dh, dw, sh, sw, 1 if flip else 0, dt, _lib.stream_ptr()), "ymi_scale_view")
    return dst[..., :3].permute(0, 3, 1, 2).contiguous()


def postprocess_logits_tta(view_outputs: Sequence[Sequence[Tensor]], scales: Sequence[float], flips: Sequence[bool], canvas_hw: Sequence[int], strides: Sequence[float],
                           anchors: Sequence[Sequence[float]], num_classes: int, score_thresh: float, nms_thresh: float, detections_per_img: int,
                           cand_cap: Optional[int] = None, multi_label: bool = True, agnostic: bool = False, classes: Optional[Sequence[int]] = None, merge: bool = False,
                           merge_redundant: bool = True) -> List[Dict[str, Tensor]]:
    """The post-process of augmented inference (ultralytics' _forward_augment, yolort/v5/models/yolo.py:152-163) on reference-layout head outputs: view_outputs[v] =
    [(N, 3, H, W, K)] per level of view v (the model's outputs on the view canvas of scale scales[v], mirrored left-right when flips[v]); canvas_hw = the full canvas.
    Every view is decoded, its boxes are brought back to the full canvas (/ scale, W - x for a mirrored view), view 0 loses its coarsest level and the last view its
    finest, and ONE NMS runs over the union (ymi_post_begin, ymi_post_decode_view per view, ymi_post_finish).  The keyword arguments are postprocess_logits's."""
    classes = _lib.normalize_classes(classes, num_classes)
    _lib.load(require_gpu=True)
    if len(view_outputs) != len(scales) or len(scales) != len(flips) or not view_outputs:
        raise ValueError("postprocess_logits_tta: one scale and one flip per view")
    h0 = view_outputs[0][0]
    if not h0.is_cuda:
        raise YmiError("postprocess runs on an MI355X only (no CPU fallback)")
    n = h0.shape[0]
    k = num_classes + 5
    cs = (3 * k + 3) // 4 * 4
    plan_inputs = []
    for outs in view_outputs:
        lv = []
        for ho in outs:
            if ho.shape[0] != n or ho.shape[1] != 3 or ho.shape[-1] != k:
                raise YmiError(f"expected ({n},3,H,W,{k}) head outputs, got {tuple(ho.shape)}")
            nhwc = torch.zeros(n, ho.shape[2], ho.shape[3], cs, device=ho.device, dtype=torch.float32)
            nhwc[..., : 3 * k] = ho.to(torch.float32).permute(0, 2, 3, 1, 4).reshape(n, ho.shape[2], ho.shape[3], 3 * k)
            lv.append(nhwc)
        plan_inputs.append(lv)
    cap = cand_cap or max(4096, 2048 * n)
    flags = (0 if multi_label else _lib.POST_BEST_CLASS) | (_lib.POST_AGNOSTIC if agnostic else 0) | _lib.merge_flags(merge, merge_redundant)
    while True:
        plan = Plan(h0.device, torch.float16)
        views = [[View(t.view(-1), 0, n, t.shape[1], t.shape[2], 3 * k, t.shape[3]) for t in lv] for lv in plan_inputs]
        pb = plan.postprocess_tta(views, scales, flips, int(canvas_hw[1]), strides, anchors, num_classes, score_thresh, nms_thresh, detections_per_img, cap, flags=flags, classes=classes)
        plan.run()
        st = pb.status.cpu().tolist()
        if st[1] == 0:
            break
        if not st[1] & 1:
            flags |= _lib.POST_EXACT_FULL
            continue
        need = max(st[0], st[3] * n)
        cap = max(int(need * 1.25) + 1024, 2 * cap)
        cap = n * (1 << ((cap + n - 1) // n - 1).bit_length())
    counts = pb.count.cpu().tolist()
    return slab_to_list(pb.boxes, pb.scores, pb.labels, counts)


class PackedLinear(NamedTuple):
    """A linear layer as ymi_classify_head reads it: weight (ceil(N / 32) * 32, K) of the compute dtype, K-contiguous, rows >= N zero; fp32 bias padded alike"""
    weight: Tensor
    bias: Tensor
    out_features: int
    in_features: int


def pack_linear(weight: Tensor, bias: Optional[Tensor], dtype: torch.dtype) -> PackedLinear:
    """nn.Linear's (N, K) weight -- or a 1x1 Conv2d's (N, K, 1, 1) -- and bias packed once for ops.classify_head: one rounding of every weight to `dtype`"""
    if weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1):
        weight = weight.reshape(weight.shape[0], weight.shape[1])
    if weight.dim() != 2:
        raise YmiError(f"pack_linear: expected an (N, K) weight or an (N, K, 1, 1) one, got {tuple(weight.shape)}")
    if dtype not in (torch.float16, torch.bfloat16):
        raise YmiError(f"classify_head computes in float16 or bfloat16 (got {dtype}): the fp32 parity mode has no classifier head")
    n, k = int(weight.shape[0]), int(weight.shape[1])
    n_pad = (n + 31) // 32 * 32
    w = torch.zeros((n_pad, k), device=weight.device, dtype=dtype)
    w[:n] = weight.detach().to(dtype)
    b = torch.zeros(n_pad, device=weight.device, dtype=torch.float32)
    if bias is not None:
        b[:n] = bias.detach().to(torch.float32)
    return PackedLinear(w, b, n, k)


def _pooled_map(m, dtype: torch.dtype):
    """a map of classify_head -> (keep-alive, pointer, n, pixels, c, pixel stride): an engine.View, or an NHWC tensor (n, h, w, c) that may be a channel slice"""
    if isinstance(m, View):
        if m.dtype != dtype:
            raise YmiError(f"classify_head: a map of {m.dtype} for a head computing in {dtype}")
        return m.base, m.ptr, m.n, m.h * m.w, m.c, m.cs
    if not isinstance(m, Tensor) or m.dim() != 4:
        raise YmiError("classify_head: a map is an engine.View or an NHWC tensor (n, h, w, c)")
    if not m.is_cuda:
        raise YmiError("classify_head runs on an MI355X only (no CPU fallback)")
    if m.dtype != dtype:
        raise YmiError(f"classify_head: a map of {m.dtype} for a head computing in {dtype}")
    n, h, w, c = (int(v) for v in m.shape)
    cs = m.stride(2) if w > 1 else (m.stride(1) if h > 1 else (m.stride(0) if n > 1 else c))
    want = (h * w * cs, w * cs, cs, 1)
    if cs < c or cs % 8 or m.data_ptr() % 16 or any(size > 1 and st != ws for size, st, ws in zip(m.shape, m.stride(), want)):
        m, cs = m.contiguous(), c
    return m, m.data_ptr(), n, h * w, c, cs


def classify_head(maps, w1, b1: Optional[Tensor] = None, w2=None, b2: Optional[Tensor] = None, *, dtype: torch.dtype = torch.float16, n_split: int = 0,
                  out: Optional[Tensor] = None, hidden: Optional[Tensor] = None) -> Tensor:
    """The tail of a classifier on the MI355X (ymi_classify_head, include/yolort_amd.h, where the arithmetic is written out): global average pool of one NHWC map or of
    up to four (their channels side by side, torch.cat(..., 1)), then Linear -- `Classify`'s head, ONE launch -- or Linear, Hardswish, Linear -- DarkNetV4 / V6's
    `avgpool` + `classifier` in eval, TWO launches.  maps: engine.Views or NHWC tensors (n, h, w, c) of `dtype` (fp16 / bf16), channel slices of a wider buffer
    included, c a multiple of 8; w1 / w2: (N, K) weights (an (N, K, 1, 1) conv weight likewise) with biases b1 / b2, or `pack_linear` results (packed once, as the
    models cache them).  -> fp32 logits (n, N_last) on the device, NO synchronisation.  n_split: see the header (0 = the launcher's rule).  out / hidden: contiguous
    device buffers to write the logits (n, N_last) fp32 / the hidden activations (n, N) of `dtype` into (allocated when None).  No CPU fallback; fp32 as the compute
    dtype (the parity mode) is refused."""
    lib = _lib.load(require_gpu=True)
    maps = list(maps) if isinstance(maps, (list, tuple)) else [maps]
    if not 1 <= len(maps) <= _lib.CLASSIFY_MAX_MAPS:
        raise YmiError(f"classify_head: {len(maps)} maps (1 .. {_lib.CLASSIFY_MAX_MAPS})")
    if dtype not in (torch.float16, torch.bfloat16):
        raise YmiError(f"classify_head computes in float16 or bfloat16 (got {dtype}): the fp32 parity mode has no classifier head")
    p1 = w1 if isinstance(w1, PackedLinear) else pack_linear(w1, b1, dtype)
    p2 = None if w2 is None else (w2 if isinstance(w2, PackedLinear) else pack_linear(w2, b2, dtype))
    views = [_pooled_map(m, dtype) for m in maps]
    n = views[0][2]
    if any(v[2] != n for v in views):
        raise YmiError(f"classify_head: the maps have {[v[2] for v in views]} rows")
    if sum(v[4] for v in views) != p1.in_features or (p2 is not None and p2.in_features != p1.out_features):
        raise YmiError(f"classify_head: {sum(v[4] for v in views)} channels into a ({p1.out_features}, {p1.in_features}) weight" + (f", then ({p2.out_features}, {p2.in_features})" if p2 else ""))
    if any(p.weight.dtype != dtype or not p.weight.is_cuda for p in (p1, p2) if p is not None):
        raise YmiError(f"classify_head: the packed weights must be {dtype} tensors on the device")
    dev = p1.weight.device
    d = _lib.ClassifyDesc()
    for i, (_, ptr, _, hw, c, cs) in enumerate(views):
        d.maps[i], d.hw[i], d.c[i], d.cs[i] = ptr, hw, c, cs
    d.num_maps, d.n, d.n1, d.dtype, d.n_split = len(views), n, p1.out_features, _lib.dtype_code(dtype), int(n_split)
    d.w1, d.b1 = p1.weight.data_ptr(), p1.bias.data_ptr()
    logits = torch.empty((n, (p2 or p1).out_features), device=dev, dtype=torch.float32) if out is None else out
    if p2 is not None and hidden is None:
        hidden = torch.empty((n, p1.out_features), device=dev, dtype=dtype)
    for t, shape, dt in ((logits, (n, (p2 or p1).out_features), torch.float32), (hidden, (n, p1.out_features), dtype)):
        if t is not None and (not t.is_cuda or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous()):
            raise YmiError(f"classify_head: an output buffer must be a contiguous device tensor of shape {shape} and dtype {dt}")
    if p2 is not None:
        d.mode, d.n2, d.w2, d.b2, d.hidden = _lib.CLASSIFY_HIDDEN_LOGITS, p2.out_features, p2.weight.data_ptr(), p2.bias.data_ptr(), hidden.data_ptr()
    d.logits = logits.data_ptr()
    check(lib.ymi_classify_head(C.byref(d), _lib.stream_ptr()), "ymi_classify_head")
    return logits


def _raise_filter_status(bits: int) -> None:
    if bits & _lib.FILTER_STATUS_BAD_COUNT:
        raise ValueError("second_stage_filter: a count of the slab lies outside [0, K]")
    if bits & (_lib.FILTER_STATUS_TOTAL | _lib.FILTER_STATUS_CAPACITY):
        raise ValueError("second_stage_filter: the crops' total disagrees with the slab's counts, or the logits hold fewer rows than the slab has detections")


def second_stage_filter(boxes: Tensor, scores: Tensor, labels: Tensor, counts: Tensor, logits: Tensor, total: Tensor, *, class_map: Optional[Tensor] = None):
    """The last line of the reference's apply_classifier (yolort/v5/utils/general.py:721-722) on the slab, on the MI355X in one launch (ymi_second_stage_filter): a
    detection survives iff the arg-max of its second-stage logits row -- through `class_map` (int32 [nc2], second-stage class -> detector label; None = the identity)
    -- equals its label.  boxes (n, K, 4), scores (n, K), labels (n, K), counts (n,): the slab; logits (capacity, nc2) fp32 in ops.crop_detections' row order and that
    call's `total`.  -> (boxes, scores, labels, counts, cls2, status): the filtered slab (same shapes, kept rows in slab order, slots past a new count zero), cls2
    (n, K) int32 = the second-stage class of every ORIGINAL detection (-1 where there is none) and the int32 status word on the device (_lib.FILTER_STATUS_*;
    `_raise_filter_status` turns it into an exception once it has been read).  Ties go to the lowest class, a NaN beats every number (torch.argmax on the CPU).
    NO synchronisation, no CPU fallback."""
    lib = _lib.load(require_gpu=True)
    ins = (boxes, scores, labels, counts, logits, total) + (() if class_map is None else (class_map,))
    if not all(t.is_cuda for t in ins):
        raise YmiError("second_stage_filter runs on an MI355X only (no CPU fallback)")
    n = int(counts.shape[0])
    if boxes.dim() != 3 or boxes.shape[0] != n or boxes.shape[2] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2]) or tuple(labels.shape) != tuple(boxes.shape[:2]) or counts.dim() != 1:
        raise YmiError(f"second_stage_filter: expected the slab (n, K, 4) / (n, K) / (n, K) / (n,), got {tuple(boxes.shape)} {tuple(scores.shape)} {tuple(labels.shape)} {tuple(counts.shape)}")
    if logits.dim() != 2 or logits.shape[1] < 1 or total.numel() < 1 or (class_map is not None and tuple(class_map.shape) != (logits.shape[1],)):
        raise YmiError(f"second_stage_filter: expected logits (capacity, nc2), total [2] and class_map (nc2,), got {tuple(logits.shape)} {tuple(total.shape)}")
    k, dev = int(boxes.shape[1]), boxes.device
    b = boxes.detach().to(torch.float32).contiguous()
    s = scores.detach().to(torch.float32).contiguous()
    l = labels.detach().to(torch.int64).contiguous()
    c = counts.detach().to(torch.int32).contiguous()
    lg = logits.detach().to(torch.float32).contiguous()
    tt = total.detach().to(torch.int32).contiguous()
    cm = None if class_map is None else class_map.detach().to(torch.int32).contiguous()
    ob, os_, ol, oc = torch.empty_like(b), torch.empty_like(s), torch.empty_like(l), torch.empty_like(c)
    cls2 = torch.empty((n, k), device=dev, dtype=torch.int32)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    d = _lib.FilterDesc()
    d.boxes, d.scores, d.labels, d.counts, d.logits, d.total = b.data_ptr(), s.data_ptr(), l.data_ptr(), c.data_ptr(), lg.data_ptr(), tt.data_ptr()
    d.class_map = None if cm is None else cm.data_ptr()
    d.out_boxes, d.out_scores, d.out_labels, d.out_counts, d.cls2, d.status = ob.data_ptr(), os_.data_ptr(), ol.data_ptr(), oc.data_ptr(), cls2.data_ptr(), status.data_ptr()
    d.n, d.k, d.cap, d.nc2 = n, k, int(lg.shape[0]), int(lg.shape[1])
    check(lib.ymi_second_stage_filter(C.byref(d), _lib.stream_ptr()), "ymi_second_stage_filter")
    return ob, os_, ol, oc, cls2, status


def _pixel_stride(t: Tensor) -> Optional[int]:
    """the pixel stride of an (n, S, c) / (n, H, W, c) tensor that is one NHWC view -- channels contiguous, every outer dimension a whole multiple of the next -- or None"""
    if t.stride(-1) != 1 and t.shape[-1] > 1:
        return None
    lead = [(size, st) for size, st in zip(t.shape[:-1], t.stride()[:-1]) if size > 1]
    cs = lead[-1][1] if lead else t.shape[-1]
    span = cs
    for size, st in reversed(lead):
        if st != span:
            return None
        span *= size
    return cs if cs >= t.shape[-1] and cs % 8 == 0 and t.data_ptr() % 16 == 0 else None


def attention(q: Tensor, k: Tensor, v: Tensor, heads: int, scale: Optional[float] = None) -> Tensor:
    """Multi-head self-attention on the MI355X: out[n, i, h] = softmax_j(scale * q[n, i, h] . k[n, j, h]) @ v[n, j, h] (ymi_attention, csrc/attention.hip; contract
    and arithmetic in include/yolort_amd.h).  q, k, v: float16 / bfloat16 device tensors of one shape (n, S, c) or (n, H, W, c), heads of d = c / heads in
    {32, 64, 128} channels side by side; scale defaults to d ** -0.5.  Strided views are read in place when they are NHWC views (contiguous channels, a pixel
    stride that is a multiple of 8, a 16-byte aligned start) -- three slices of one qkv tensor are; anything else is copied once.  Returns a contiguous tensor of
    q's shape.  One launch on the current stream, no synchronisation, no CPU fallback."""
    lib = _lib.load(require_gpu=True)
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise YmiError("attention runs on an MI355X only (no CPU fallback)")
    if q.dim() not in (3, 4) or k.shape != q.shape or v.shape != q.shape or k.dtype != q.dtype or v.dtype != q.dtype:
        raise YmiError(f"attention: q, k, v must share one shape (n, S, c) or (n, H, W, c) and one dtype, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise YmiError(f"attention computes in float16 or bfloat16, got {q.dtype}")
    n, c = q.shape[0], q.shape[-1]
    tokens = q.numel() // max(n * c, 1)
    if heads < 1 or c % heads or c // heads not in _lib.ATTN_HEAD_DIMS:
        raise YmiError(f"attention: {c} channels in {heads} heads: the head dimension must be one of {_lib.ATTN_HEAD_DIMS}")
    ts = [t.detach() if _pixel_stride(t) is not None else t.detach().contiguous() for t in (q, k, v)]
    out = torch.empty(q.shape, device=q.device, dtype=q.dtype)
    d = _lib.AttnDesc(q=ts[0].data_ptr(), k=ts[1].data_ptr(), v=ts[2].data_ptr(), o=out.data_ptr(), n=n, S=tokens, heads=heads, d=c // heads, c=c,
                      q_cstride=_pixel_stride(ts[0]), k_cstride=_pixel_stride(ts[1]), v_cstride=_pixel_stride(ts[2]), o_cstride=c, dtype=_lib.dtype_code(q.dtype),
                      scale=float(c // heads) ** -0.5 if scale is None else float(scale))
    with torch.cuda.device(q.device):
        check(lib.ymi_attention(C.byref(d), _lib.stream_ptr()), "ymi_attention")
    return out


def _nhwc_of(t: Tensor, align: int):
    """(the (n, h, w, c) view of an NCHW tensor, its pixel stride): read in place when the memory already is one NHWC view (channels_last, or a channel slice of
    one) with a 16-byte aligned start and a pixel stride that is a multiple of `align`; copied once otherwise"""
    v = t.detach().permute(0, 2, 3, 1)
    n, h, w, c = v.shape
    cs = v.stride(2)
    if v.numel() == 0 or not (v.stride(3) == 1 and cs >= c and cs % align == 0 and v.stride(1) == w * cs and v.stride(0) == h * w * cs and v.data_ptr() % 16 == 0):
        v, cs = v.contiguous(), c
    return v, cs


def quantize_int8(x: Tensor, scale: float) -> Tensor:
    """q = clamp(rint(x / scale), -127, 127) as int8: the per-tensor symmetric quantisation that feeds conv2d_int8 (ymi_quantize_i8, csrc/conv_i8.hip; NaN -> 0, ties
    to even).  x: float16 / bfloat16 / float32 NCHW device tensor.  Returns an int8 NCHW tensor in channels_last memory (the NHWC layout the convolution reads in
    place).  One launch on the current stream (a source that is not channels_last is first copied into that layout by torch); no CPU fallback."""
    lib = _lib.load(require_gpu=True)
    if not x.is_cuda:
        raise YmiError("quantize_int8 runs on an MI355X only (no CPU fallback)")
    if x.dim() != 4 or x.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise YmiError(f"quantize_int8: a float16 / bfloat16 / float32 NCHW tensor is needed, got {x.dtype} {tuple(x.shape)}")
    xv, xcs = _nhwc_of(x, 1)
    n, h, w, c = xv.shape
    out = torch.empty((n, h, w, c), device=x.device, dtype=torch.int8)
    d = _lib.QuantI8Desc(x=xv.data_ptr(), y=out.data_ptr(), npix=n * h * w, c=c, x_cstride=xcs, y_cstride=c,
                         dtype=_lib.dtype_code(x.dtype), scale=float(scale))
    with torch.cuda.device(x.device):
        check(lib.ymi_quantize_i8(C.byref(d), _lib.stream_ptr()), "ymi_quantize_i8")
    return out.permute(0, 3, 1, 2)


def conv2d_int8(xq: Tensor, packed, stride: int = 1, act: int = _lib.ACT_SILU, out_scale: Optional[float] = None, res: Optional[Tensor] = None, res_scale: float = 1.0,
                dtype: torch.dtype = torch.float16) -> Tensor:
    """INT8 convolution with the requantising epilogue y = requant(act(acc * scale + bias) + res_scale * res) (ymi_conv2d_i8, csrc/conv_i8.hip; the arithmetic is the
    contract in include/yolort_amd.h).  xq: int8 NCHW device tensor (quantize_int8 makes one); packed: engine.PackedConvI8 (k in {1, 3}, padding k // 2); stride 1 / 2;
    act: an _lib.ACT_* code.  With `out_scale` the result is int8 (codes of y / out_scale), else `dtype` (float16 / bfloat16); `res` is an NCHW tensor of the result's
    shape and type.  Returns an NCHW tensor in channels_last memory.  One launch on the current stream; no CPU fallback."""
    lib = _lib.load(require_gpu=True)
    if not xq.is_cuda:
        raise YmiError("conv2d_int8 runs on an MI355X only (no CPU fallback)")
    if xq.dim() != 4 or xq.dtype != torch.int8 or xq.shape[1] != packed.cin:
        raise YmiError(f"conv2d_int8: an int8 NCHW tensor of {packed.cin} channels is needed, got {xq.dtype} {tuple(xq.shape)}")
    odt = torch.int8 if out_scale is not None else dtype
    if odt not in (torch.int8, torch.float16, torch.bfloat16):
        raise YmiError(f"conv2d_int8: the output is int8 (with out_scale), float16 or bfloat16, got {odt}")
    xv, xcs = _nhwc_of(xq, 16)
    n, h, w, _ = xv.shape
    k = packed.k
    ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
    out = torch.empty((n, ho, wo, packed.cout), device=xq.device, dtype=odt)
    rv, rcs = None, 0
    if res is not None:
        if tuple(res.shape) != (n, packed.cout, ho, wo) or res.dtype != odt:
            raise YmiError(f"conv2d_int8: the shortcut must be {(n, packed.cout, ho, wo)} of {odt}, got {tuple(res.shape)} of {res.dtype}")
        rv, rcs = _nhwc_of(res, 8)
    d = _lib.ConvI8Desc(x=xv.data_ptr(), w=packed.w.data_ptr(), scale=packed.scale.data_ptr(), bias=packed.bias.data_ptr(), y=out.data_ptr(), res=None if rv is None else rv.data_ptr(),
                        n=n, h=h, w_in=w, cin=packed.cin, x_cstride=xcs, ho=ho, wo=wo, cout=packed.cout, y_cstride=packed.cout,
                        res_cstride=rcs, k=k, s=stride, p=k // 2, act=act, out_dtype=_lib.dtype_code(odt),
                        out_scale=0.0 if out_scale is None else float(out_scale), res_scale=float(res_scale))
    with torch.cuda.device(xq.device):
        check(lib.ymi_conv2d_i8(C.byref(d), _lib.stream_ptr()), "ymi_conv2d_i8")
    return out.permute(0, 3, 1, 2)
