"""Op-level Python wrappers over the C ABI (tests, stand-alone API pieces).  No fallbacks."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

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
