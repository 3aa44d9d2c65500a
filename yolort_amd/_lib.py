"""ctypes binding of libyolort_amd.so (C ABI in include/yolort_amd.h).

There is NO fallback: if the shared library is missing or no MI355X is visible, every compute
entry point raises.  `import torch` happens first on purpose: the torch wheel bundles its own
libamdhip64.so (same SONAME as /opt/rocm's), and loading ours afterwards makes the dynamic loader
bind our HIP symbols to the runtime torch already initialised, so streams, events and device
pointers are shared (SURVEY.md section 7 "Two ROCm runtimes in one process").
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch  # noqa: F401  (must precede CDLL, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("YOLORT_AMD_LIB") or os.path.join(_HERE, "lib", "libyolort_amd.so")   # override: tuning builds only

YMI_F16, YMI_BF16, YMI_F32, YMI_U8 = 0, 1, 2, 3
YMI_U8_HWC = 4   # ymi_letterbox input only: interleaved (h, w, 3) uint8
ACT_NONE, ACT_SILU, ACT_HARDSWISH, ACT_LEAKY = 0, 1, 2, 3   # include/yolort_amd.h YMI_ACT_*: the last two belong to the legacy r3.1 blocks
MAX_LEVELS = 4


class YmiError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("ktab", C.c_void_p), ("y", C.c_void_p), ("res", C.c_void_p),
        ("n", C.c_int32), ("h", C.c_int32), ("w_in", C.c_int32), ("cin", C.c_int32), ("x_cstride", C.c_int32),
        ("ho", C.c_int32), ("wo", C.c_int32), ("cout", C.c_int32), ("cout_pad", C.c_int32), ("y_cstride", C.c_int32), ("res_cstride", C.c_int32),
        ("kh", C.c_int32), ("kw", C.c_int32), ("sh", C.c_int32), ("sw", C.c_int32), ("ph", C.c_int32), ("pw", C.c_int32), ("k_pad", C.c_int32),
        ("act", C.c_int32), ("dtype", C.c_int32), ("out_dtype", C.c_int32), ("tile", C.c_int32),
        ("y2", C.c_void_p), ("y2_cstride", C.c_int32), ("cout_split", C.c_int32),
        ("y2_mode", C.c_int32), ("reserved0", C.c_int32),
        ("chain_w", C.c_void_p), ("chain_bias", C.c_void_p), ("chain_y", C.c_void_p), ("chain_cout", C.c_int32), ("chain_y_cstride", C.c_int32),
        ("chain_x2", C.c_void_p), ("chain_x2_cstride", C.c_int32), ("chain_k2", C.c_int32),
        ("zeros", C.c_void_p),
    ]


class C3Desc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("w12", C.c_void_p), ("b12", C.c_void_p), ("wm1", C.c_void_p), ("bm1", C.c_void_p),
        ("wm2", C.c_void_p), ("bm2", C.c_void_p), ("w3", C.c_void_p), ("b3", C.c_void_p),
        ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("x_cstride", C.c_int32), ("y_cstride", C.c_int32), ("dtype", C.c_int32),
        ("c_in", C.c_int32), ("c_hidden", C.c_int32), ("c_out", C.c_int32), ("n_bottlenecks", C.c_int32), ("shortcut", C.c_int32),
        ("k12_pad", C.c_int32), ("km1_pad", C.c_int32), ("km2_pad", C.c_int32), ("k3_pad", C.c_int32), ("mode", C.c_int32),
        # ABI 6: the strip kernel (csrc/c3_tile.hip)
        ("wblob", C.c_void_p), ("y1_in", C.c_void_p), ("y1_out", C.c_void_p), ("y2", C.c_void_p),
        ("y1_in_cstride", C.c_int32), ("y1_out_cstride", C.c_int32), ("y2_cstride", C.c_int32), ("reserved1", C.c_int32),
    ]


class PlanRegion(C.Structure):
    _fields_ = [("base", C.c_void_p), ("bytes", C.c_int64), ("kind", C.c_int32), ("tag", C.c_int32)]


REGION_CONST, REGION_SCRATCH, REGION_IO = 1, 2, 3
TAG_NONE, TAG_INPUT, TAG_RESCALE, TAG_BOXES, TAG_SCORES, TAG_LABELS, TAG_STATUS_COUNT, TAG_SLAB = range(8)
ABI_VERSION = 6   # include/yolort_amd.h YMI_ABI_VERSION
POST_EXACT_FULL = 1
POST_BEST_CLASS = 2   # YMI_POST_BEST_CLASS: one label per anchor (ultralytics' multi_label=False)
POST_AGNOSTIC = 4     # YMI_POST_AGNOSTIC: one NMS over all boxes of an image, whatever their label (ultralytics' agnostic=True)
POST_CLASS_FILTER = 8  # YMI_POST_CLASS_FILTER: only candidates of the classes in the workspace's mask (ultralytics' classes=[...])
POST_MERGE = 16        # YMI_POST_MERGE: merge-NMS, a kept box becomes the score-weighted mean of the candidates it overlaps (ultralytics' merge = True); images of 1 < n < 3000 candidates
POST_MERGE_KEEP_SINGLE = 32   # YMI_POST_MERGE_KEEP_SINGLE (with POST_MERGE only): keep the boxes that have no contributor but themselves (ultralytics' redundant = False)


def merge_flags(merge: bool, merge_redundant: bool = True) -> int:
    """the YMI_POST_MERGE* bits of `merge=` / `merge_redundant=` (merge_redundant only matters with merge)"""
    return (POST_MERGE | (0 if merge_redundant else POST_MERGE_KEEP_SINGLE)) if merge else 0


class PostDesc(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p * MAX_LEVELS),
        ("lh", C.c_int32 * MAX_LEVELS), ("lw", C.c_int32 * MAX_LEVELS), ("lcstride", C.c_int32 * MAX_LEVELS),
        ("stride", C.c_float * MAX_LEVELS),
        ("anchors", (C.c_float * 6) * MAX_LEVELS),
        ("num_levels", C.c_int32), ("n", C.c_int32), ("num_classes", C.c_int32),
        ("score_thresh", C.c_float), ("nms_thresh", C.c_float),
        ("detections_per_img", C.c_int32),
        ("rescale", C.c_void_p),
        ("out_boxes", C.c_void_p), ("out_scores", C.c_void_p), ("out_labels", C.c_void_p), ("out_count", C.c_void_p),
        ("status", C.c_void_p),
        ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
        ("cand_cap", C.c_int32),
        ("flags", C.c_int32),
        ("out_slab", C.c_void_p),   # ABI 5: packed wire slab (n, 6K + 1) fp32 or NULL
    ]


class PostView(C.Structure):
    """ymi_post_view: one view of augmented inference for ymi_post_decode_view (its levels, the levels to skip, its anchor base, scale and mirror width)"""
    _fields_ = [
        ("logits", C.c_void_p * MAX_LEVELS),
        ("lh", C.c_int32 * MAX_LEVELS), ("lw", C.c_int32 * MAX_LEVELS), ("lcstride", C.c_int32 * MAX_LEVELS),
        ("stride", C.c_float * MAX_LEVELS),
        ("anchors", (C.c_float * 6) * MAX_LEVELS),
        ("num_levels", C.c_int32), ("skip_mask", C.c_int32), ("anchor_base", C.c_int32),
        ("scale", C.c_float), ("flip_w", C.c_int32), ("reserved", C.c_int32),
    ]


EVAL_MAX_THRS, EVAL_MAX_RNGS, EVAL_MAX_PER_IMAGE = 16, 4, 1024   # YMI_EVAL_MAX_*
EVAL_STATUS_BAD_LABEL, EVAL_STATUS_STALE_ROW = 1, 2                # YMI_EVAL_STATUS_*: bits of status[1]


class EvalDesc(C.Structure):
    """ymi_eval_desc: the detection slab, the padded ground truth, the outputs and the protocol (thresholds, area ranges, max_dets) of one ymi_eval_match launch"""
    _fields_ = [
        ("boxes", C.c_void_p), ("scores", C.c_void_p), ("labels", C.c_void_p), ("counts", C.c_void_p),
        ("gt_boxes", C.c_void_p), ("gt_labels", C.c_void_p), ("gt_counts", C.c_void_p),
        ("tp", C.c_void_p), ("ig", C.c_void_p), ("rank", C.c_void_p), ("n_gt", C.c_void_p), ("status", C.c_void_p),
        ("thrs", C.c_double * EVAL_MAX_THRS), ("area_rng", (C.c_float * 2) * EVAL_MAX_RNGS),
        ("n", C.c_int32), ("k", C.c_int32), ("g", C.c_int32), ("num_thrs", C.c_int32), ("num_rngs", C.c_int32),
        ("max_dets", C.c_int32), ("num_classes", C.c_int32), ("reserved", C.c_int32),
    ]


CROP_STATUS_CAPACITY, CROP_STATUS_BAD_COUNT = 1, 2   # YMI_CROP_STATUS_*: bits of total[1]


class CropDesc(C.Structure):
    """ymi_crop_desc: the images (host arrays of device pointers and sizes), the detection slab, the outputs and the parameters of one ymi_crop_resize call"""
    _fields_ = [
        ("imgs", C.POINTER(C.c_void_p)), ("hw", C.POINTER(C.c_int32)), ("boxes", C.c_void_p), ("counts", C.c_void_p),
        ("crops", C.c_void_p), ("index", C.c_void_p), ("total", C.c_void_p),
        ("mean", C.c_float * 3), ("std", C.c_float * 3), ("gain", C.c_float), ("pad", C.c_float),
        ("n", C.c_int32), ("k", C.c_int32), ("cap", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
        ("in_dtype", C.c_int32), ("out_dtype", C.c_int32), ("square", C.c_int32), ("normalize", C.c_int32), ("reserved", C.c_int32),
    ]


RENDER_MAX_K, RENDER_NAME_STRIDE = 1024, 28   # YMI_RENDER_MAX_K, YMI_RENDER_NAME_STRIDE
RENDER_STATUS_BAD_COUNT, RENDER_STATUS_STALE_ROW, RENDER_STATUS_BAD_LABEL = 1, 2, 4   # YMI_RENDER_STATUS_*: bits of the status word


class RenderDesc(C.Structure):
    """ymi_render_desc: the images (host arrays of device pointers, sizes, outline widths and font scales), the detection slab, the name and colour tables and the
    flags of one ymi_render call"""
    _fields_ = [
        ("imgs", C.POINTER(C.c_void_p)), ("hw", C.POINTER(C.c_int32)), ("lw", C.POINTER(C.c_int32)), ("fs", C.POINTER(C.c_int32)),
        ("boxes", C.c_void_p), ("scores", C.c_void_p), ("labels", C.c_void_p), ("counts", C.c_void_p), ("names", C.c_void_p), ("colors", C.c_void_p), ("status", C.c_void_p),
        ("m", C.c_int32), ("txt_color", C.c_int32 * 3), ("num_classes", C.c_int32), ("in_dtype", C.c_int32), ("draw_labels", C.c_int32), ("draw_conf", C.c_int32),
        ("n", C.c_int32), ("k", C.c_int32), ("reserved", C.c_int32),
    ]


VIEW_PAD = 0.447  # YMI_VIEW_PAD: the pad value of a view canvas (scale_img's F.pad value)
TTA_SCALES, TTA_FLIPS = (1.0, 0.83, 0.67), (False, True, False)   # ultralytics' _forward_augment (yolort/v5/models/yolo.py:154-155): scales, left-right mirror


def tta_view_size(h: int, w: int, ratio: float, gs: int = 32):
    """scale_img's sizes (yolort/v5/utils/torch_utils.py:296-299) in Python floats, exactly as the reference computes them: the resized size (sh, sw) and the
    gs-multiple canvas (H', W') it is padded into; ratio 1.0 is the canvas itself"""
    import math
    if ratio == 1.0:
        return (h, w), (h, w)
    return (int(h * ratio), int(w * ratio)), (math.ceil(h * ratio / gs) * gs, math.ceil(w * ratio / gs) * gs)


def tta_layout(view_levels, num_views=None):
    """The concatenated anchor axis of augmented inference (_clip_augmented, yolo.py:199-208): view_levels[v] = [(h, w)] per pyramid level of view v.  View 0 drops its
    coarsest level, the last view its finest; skipped levels occupy no indices.  Returns ([(skip_mask, anchor_base)] per view, total anchors)."""
    nv = len(view_levels)
    out, base = [], 0
    for v, levels in enumerate(view_levels):
        nl = len(levels)
        skip = 0
        if nv > 1 and v == 0:
            skip |= 1 << (nl - 1)
        if nv > 1 and v == nv - 1:
            skip |= 1
        out.append((skip, base))
        base += sum(3 * h * w for l, (h, w) in enumerate(levels) if not (skip >> l) & 1)
    return out, base


_SIGS = {
    "ymi_abi_version": (C.c_int, []),
    "ymi_last_error": (C.c_char_p, []),
    "ymi_device_count": (C.c_int, []),
    "ymi_letterbox": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "ymi_nchw_to_nhwc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ymi_nhwc_to_nchw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "ymi_conv2d": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    "ymi_c3_fused": (C.c_int, [C.POINTER(C3Desc), C.c_void_p]),
    "ymi_plan_add_c3_fused": (C.c_int, [C.c_void_p, C.POINTER(C3Desc)]),
    "ymi_c3_blob_bytes": (C.c_int64, [C.POINTER(C3Desc)]),
    "ymi_c3_pack": (C.c_int, [C.POINTER(C3Desc), C.c_void_p, C.c_void_p]),
    "ymi_c3_tile_supported": (C.c_int, [C.POINTER(C3Desc)]),
    "ymi_c3_tile_geometry": (C.c_int, [C.POINTER(C3Desc), C.POINTER(C.c_int)]),
    "ymi_conv_stem_planar": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "ymi_stem_body1_planar": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc), C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "ymi_stem_body1": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc), C.c_void_p]),
    "ymi_clock_probe": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "ymi_conv_build_ktab": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "ymi_conv_f32_pick_tile": (C.c_int, [C.c_int, C.c_int]),
    "ymi_spp_pool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ymi_upsample2x": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ymi_copy_view": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ymi_act": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "ymi_plan_add_act": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "ymi_postprocess_ws_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "ymi_postprocess": (C.c_int, [C.POINTER(PostDesc), C.c_void_p]),
    "ymi_post_begin": (C.c_int, [C.POINTER(PostDesc), C.c_void_p]),
    "ymi_post_finish": (C.c_int, [C.POINTER(PostDesc), C.c_void_p]),
    "ymi_post_decode_view": (C.c_int, [C.POINTER(PostDesc), C.POINTER(PostView), C.c_void_p]),
    "ymi_plan_add_post_decode_view": (C.c_int, [C.c_void_p, C.POINTER(PostDesc), C.POINTER(PostView)]),
    "ymi_scale_view": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ymi_plan_add_scale_view": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ymi_post_class_mask_offset": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "ymi_post_set_classes": (C.c_int, [C.POINTER(PostDesc), C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    "ymi_plan_set_classes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    "ymi_conv_head_decode_group": (C.c_int, [C.POINTER(ConvDesc), C.c_int, C.POINTER(PostDesc), C.c_void_p]),
    "ymi_conv_head_decode": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(PostDesc), C.c_int, C.c_void_p]),
    "ymi_nms_ws_bytes": (C.c_int64, [C.c_int]),
    "ymi_batched_nms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "ymi_nms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "ymi_eval_match": (C.c_int, [C.POINTER(EvalDesc), C.c_void_p]),
    "ymi_crop_resize": (C.c_int, [C.POINTER(CropDesc), C.c_void_p]),
    "ymi_render": (C.c_int, [C.POINTER(RenderDesc), C.c_void_p]),
    "ymi_plan_create": (C.c_void_p, []),
    "ymi_plan_destroy": (None, [C.c_void_p]),
    "ymi_plan_add_conv": (C.c_int, [C.c_void_p, C.POINTER(ConvDesc)]),
    "ymi_plan_add_spp_pool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ymi_plan_add_upsample2x": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "ymi_plan_add_copy_view": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "ymi_plan_add_postprocess": (C.c_int, [C.c_void_p, C.POINTER(PostDesc)]),
    "ymi_plan_add_post_begin": (C.c_int, [C.c_void_p, C.POINTER(PostDesc)]),
    "ymi_plan_add_head_decode": (C.c_int, [C.c_void_p, C.POINTER(ConvDesc), C.POINTER(PostDesc), C.c_int]),
    "ymi_plan_add_head_decode_group": (C.c_int, [C.c_void_p, C.POINTER(ConvDesc), C.c_int, C.POINTER(PostDesc)]),
    "ymi_plan_add_post_finish": (C.c_int, [C.c_void_p, C.POINTER(PostDesc)]),
    "ymi_plan_num_ops": (C.c_int, [C.c_void_p]),
    "ymi_plan_set_fuse_stem": (C.c_int, [C.c_void_p, C.c_int]),
    "ymi_plan_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "ymi_plan_profile": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_void_p]),
    "ymi_plan_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ymi_plan_submit": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "ymi_plan_done_query": (C.c_int, [C.c_void_p]),
    "ymi_plan_done_sync": (C.c_int, [C.c_void_p]),
    "ymi_plan_export": (C.c_int, [C.c_void_p, C.POINTER(PlanRegion), C.c_int, C.c_char_p, C.c_void_p]),
    "ymi_plan_import": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(PlanRegion), C.c_int, C.POINTER(C.c_int)]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

_lib: Optional[C.CDLL] = None


def load(require_gpu: bool = False) -> C.CDLL:
    """Loads the shared library (once).  Raises YmiError loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise YmiError(
                f"{LIB_PATH} is missing: the HIP extension has not been built. Run `python -m yolort_amd._build` "
                "(needs hipcc, cross-compiles for gfx950 without a GPU). There is no CPU fallback."
            )
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if lib.ymi_abi_version() != ABI_VERSION:
            raise YmiError(f"ABI version mismatch: library reports {lib.ymi_abi_version()}, binding expects {ABI_VERSION}")
        _lib = lib
    if require_gpu:
        if not torch.cuda.is_available():
            raise YmiError("no MI355X visible (torch.cuda.is_available() is False): yolort_amd has no CPU fallback")
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc < 0:
        msg = _lib.ymi_last_error().decode("utf-8", "replace") if _lib is not None else ""
        raise YmiError(f"{what or 'libyolort_amd'} failed (code {rc}): {msg}")


def normalize_classes(classes, num_classes: Optional[int] = None):
    """the `classes=` argument of the post-process (ultralytics' non_max_suppression(..., classes=...)): None = no filter, else an iterable of class indices -> a sorted
    tuple without duplicates (order and repeats are irrelevant to a set).  ValueError for a non-integer, a negative index or, when `num_classes` is known, one >= it."""
    if classes is None:
        return None
    import operator
    if isinstance(classes, (str, bytes)):
        raise ValueError(f"classes must be an iterable of class indices, got {classes!r}")
    out = set()
    try:
        items = list(classes)
    except TypeError:
        raise ValueError(f"classes must be an iterable of class indices, got {classes!r}") from None
    for c in items:
        if isinstance(c, bool):
            raise ValueError(f"classes: {c!r} is not a class index")
        try:
            i = operator.index(c)
        except TypeError:
            raise ValueError(f"classes: {c!r} is not an integer class index") from None
        if i < 0 or (num_classes is not None and i >= num_classes):
            raise ValueError(f"classes: index {i} outside [0, {num_classes if num_classes is not None else 'num_classes'})")
        out.add(i)
    return tuple(sorted(out))


def dtype_code(dt: torch.dtype) -> int:
    try:
        return {torch.float16: YMI_F16, torch.bfloat16: YMI_BF16, torch.float32: YMI_F32, torch.uint8: YMI_U8}[dt]
    except KeyError:
        raise YmiError(f"unsupported dtype {dt}") from None


def stream_ptr(stream: Optional["torch.cuda.Stream"] = None) -> C.c_void_p:
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)
