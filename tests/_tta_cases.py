"""Shared by tests/test_tta.py (CPU: host logic and the two new kernels on the simulator) and tests/test_tta_gpu.py (the real kernels and the engine): the yardsticks of
augmented inference (include/yolort_amd.h ymi_scale_view / ymi_post_decode_view; Python `augment=True`), the case tables and ONE driver for both libraries -- the simulator
takes host pointers, libyolort_amd.so device pointers, the calls are the same.

Restated from the reference (its yolort.v5 modules are not imported: importing them tries to fetch a font):
  scale_img       yolort/v5/utils/torch_utils.py:288-300   s = (int(h * r), int(w * r)); F.interpolate(size=s, bilinear, align_corners=False); F.pad to
                                                           ceil(x * r / gs) * gs with 0.447
  _forward_augment yolort/v5/models/yolo.py:152-163        scales 1 / 0.83 / 0.67, flip 3 (left-right) for the second view; torch.cat(y, 1) after _clip_augmented
  _descale_pred   yolort/v5/models/yolo.py:181-197         xywh / scale; x = img_w - x for flip 3
  _clip_augmented yolort/v5/models/yolo.py:199-208         view 0 loses its last (coarsest) level, the last view its first (finest)
"""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

import _post_cases

F32 = np.float32
SCALES, FLIPS = (1.0, 0.83, 0.67), (False, True, False)
PAD = 0.447
GUARD = -7.0                                       # fills the guard bands around a destination / the slots of the outputs
POST_EXACT_FULL, POST_BEST_CLASS, POST_AGNOSTIC, POST_CLASS_FILTER, POST_MERGE = 1, 2, 4, 8, 16
HI, MID, OFF = 20.0, 0.0, -20.0                    # logits whose sigmoid is exactly 1.0, exactly 0.5, "fails" (tests/_merge_cases.py)
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
DT_CODE = {"f16": 0, "bf16": 1, "f32": 2}


# ---- the view canvas ---------------------------------------------------------------------------------------------------------------------------------------------
def view_sizes(h, w, ratio, gs=32):
    """torch_utils.py:296-299 -> ((sh, sw), (H', W'))"""
    return (int(h * ratio), int(w * ratio)), tuple(math.ceil(x * ratio / gs) * gs for x in (h, w))


def scale_img_ref(x, ratio, flip=False, gs=32):
    """yolo.py:158 + torch_utils.py:288-300 on an (n, 3, h, w) fp32 tensor (the stored values of the canvas, widened)"""
    x = x.flip(3) if flip else x
    (sh, sw), (dh, dw) = view_sizes(x.shape[2], x.shape[3], ratio, gs)
    img = F.interpolate(x, size=(sh, sw), mode="bilinear", align_corners=False)
    return F.pad(img, [0, dw - sw, 0, dh - sh], value=PAD)


def scale_tolerance(dt):
    """|kernel - F.interpolate in fp32| for pixels in [0, R], R = 1.  The value is h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11) with w0 + w1 = h0 + h1 = 1; both
    sides take the source index as the exact (dst + 0.5) * scale - 0.5 rounded once (a fused multiply-add), so the weights h_i, w_j are the same fp32 numbers.  The
    kernel evaluates the four tap weights w_ij = fl(h_i * w_j) (relative error u = 2^-24 each: sum_ij u w_ij |v_ij| <= u R), one rounded product and three fused
    multiply-adds, each rounding a partial sum that is <= R: 4 u R -- 5 roundings of the pixel range.  torch's own evaluation of the same expression (nested or over the
    four taps) carries 4 to 5 of them, in the other direction at worst: 10 * 2^-24.  The 16-bit modes round the fp32 value ONCE to the storage type; the comparison allows
    one storage ulp of the largest binade below R (fp16 2^-11, bf16 2^-8) on top."""
    return 10 * 2.0 ** -24 + {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}[dt]


SCALE_CASES = (   # (h, w, ratio): 64 x 96 at 0.5 is exact (every weight 0.5); at 0.83 / 0.67 the destination keeps 64 x 96 with pad bands 11 / 17 and 22 / 32; 128 x 160 -> 96 x 128
    (64, 96, 0.5), (64, 96, 0.83), (64, 96, 0.67), (128, 160, 0.67),
)


def canvas(n, h, w, dt, seed=3):
    """(n, 3, h, w) pixels in [0, 1] already rounded to the storage type, as fp32"""
    g = torch.Generator().manual_seed(seed + h + w)
    return torch.rand(n, 3, h, w, generator=g).to(TORCH_DT[dt]).float()


def run_scale(lib, x, ratio, flip, dt, gs=32, device="cpu", stream=None):
    """ymi_scale_view of the stored canvas `x` (fp32 values representable in dt) -> (destination (n, 3, H', W') widened to fp32, channel 3 (n, H', W'), the guard bands).
    The source's channel 3 holds a sentinel (it must not be read into the result), the destination is poisoned and lies between two guard bands of a row each."""
    n, _, h, w = x.shape
    (sh, sw), (dh, dw) = view_sizes(h, w, ratio, gs)
    tdt = TORCH_DT[dt]
    src = torch.full((n, h, w, 4), 0.25, dtype=tdt)
    src[..., :3] = x.permute(0, 2, 3, 1).to(tdt)
    band = dw * 4
    flat = torch.full((band + n * dh * dw * 4 + band,), GUARD, dtype=tdt)
    src, flat = src.to(device), flat.to(device)
    dst_ptr = flat.data_ptr() + band * flat.element_size()
    rc = lib.ymi_scale_view(C.c_void_p(src.data_ptr()), n, h, w, C.c_void_p(dst_ptr), dh, dw, sh, sw, 1 if flip else 0, DT_CODE[dt], stream)
    assert rc == 0, rc
    if device != "cpu":
        torch.cuda.synchronize()
    flat = flat.cpu()
    body = flat[band: band + n * dh * dw * 4].view(n, dh, dw, 4).float()
    return body[..., :3].permute(0, 3, 1, 2).contiguous(), body[..., 3], (flat[:band].float(), flat[-band:].float())


def check_scale(got, ch3, guards, x, ratio, flip, dt, gs=32):
    """the comparisons of one scale case: resized pixels within scale_tolerance (bit for bit at ratio 0.5), pad pixels, channel 3 and the guard bands exactly"""
    ref = scale_img_ref(x, ratio, flip, gs)
    (sh, sw), (dh, dw) = view_sizes(x.shape[2], x.shape[3], ratio, gs)
    assert tuple(got.shape[2:]) == (dh, dw) == tuple(ref.shape[2:])
    pad_value = torch.tensor(PAD).to(TORCH_DT[dt]).float()
    assert (got[:, :, sh:, :] == pad_value).all() and (got[:, :, :, sw:] == pad_value).all(), "pad pixels"
    assert (ch3 == 0).all(), "channel 3"
    assert (guards[0] == GUARD).all() and (guards[1] == GUARD).all(), "a row outside the destination was written"
    inside, want = got[:, :, :sh, :sw], ref[:, :, :sh, :sw]
    err = float((inside - want).abs().max())
    print(f"scale {tuple(x.shape)} r={ratio} flip={flip} {dt}: max |err| {err:.3e} (tolerance {scale_tolerance(dt):.3e})")
    if ratio == 0.5:
        assert torch.equal(inside, want.to(TORCH_DT[dt]).float()), "ratio 0.5 is exact"
    assert err <= scale_tolerance(dt), err
    return err


# ---- the views of a canvas and their pyramids ----------------------------------------------------------------------------------------------------------------------------
def view_shapes(h, w, strides):
    """per view the (h, w) of every pyramid level: the view canvases are multiples of the largest stride"""
    gs = int(max(strides))
    out = []
    for r in SCALES:
        _, (dh, dw) = view_sizes(h, w, r, gs) if r != 1.0 else (None, (h, w))
        out.append([(dh // int(s), dw // int(s)) for s in strides])
    return out


def layout(shapes):
    """_clip_augmented restated: ([(skip_mask, anchor_base)] per view, total anchors); must equal yolort_amd._lib.tta_layout"""
    out, base, nv = [], 0, len(shapes)
    for v, lv in enumerate(shapes):
        skip = (1 << (len(lv) - 1) if v == 0 and nv > 1 else 0) | (1 if v == nv - 1 and nv > 1 else 0)
        out.append((skip, base))
        base += sum(3 * h * w for l, (h, w) in enumerate(lv) if not (skip >> l) & 1)
    return out, base


def lattice_levels(n, shapes, nc, cells):
    """cells: (level, img, anchor, y, x, objectness logit, {class: logit}) -> reference-layout head outputs [(n, 3, h, w, nc + 5)] per level; box logits 0 (centre
    (x + 0.5) * stride, the anchor's size); everything not listed fails"""
    heads = []
    for h, w in shapes:
        ho = torch.zeros(n, 3, h, w, nc + 5)
        ho[..., 4:] = OFF
        heads.append(ho)
    for l, img, a, y, x, obj, cls in cells:
        heads[l][img, a, y, x, 4] = obj
        for c, v in cls.items():
            heads[l][img, a, y, x, 5 + c] = v
    return heads


def nhwc_logits(heads, nc, device="cpu"):
    kk, out = nc + 5, []
    for ho in heads:
        n, _, h, w, _ = ho.shape
        t = torch.zeros(n, h, w, (3 * kk + 3) // 4 * 4, dtype=torch.float32)
        t[..., : 3 * kk] = ho.permute(0, 2, 3, 1, 4).reshape(n, h, w, 3 * kk)
        out.append(t.to(device))
    return out


def mask_words(classes):
    m = np.zeros(128, np.uint32)
    for c in classes:
        m[c >> 5] |= np.uint32(1 << (c & 31))
    return m


def run_views(lib, views, n, nc, strides, anchors, thr, nms, k, cap, flags=0, classes=None, device="cpu", stream=None, plain=False):
    """ymi_post_begin, one ymi_post_decode_view per entry of `views`, ymi_post_finish, on a dirty workspace and pre-filled outputs.
    views: dicts(heads=[(n, 3, h, w, nc + 5)] per level, skip, base, scale, flip_w).  The sink is one pseudo-level of 1 x (A / 3), A = what the views cover.
    plain=True: ONE view through ymi_postprocess instead (the library's own scale-1 decode of the same logits).  -> dict of CPU tensors"""
    from yolort_amd._lib import PostDesc, PostView
    total = 0
    for v in views:
        kept = sum(3 * ho.shape[2] * ho.shape[3] for l, ho in enumerate(v["heads"]) if not (v.get("skip", 0) >> l) & 1)
        total = max(total, v.get("base", 0) + kept)
    lib.ymi_postprocess_ws_bytes.argtypes, lib.ymi_postprocess_ws_bytes.restype = [C.c_int, C.c_int, C.c_int], C.c_int64
    lib.ymi_post_class_mask_offset.argtypes, lib.ymi_post_class_mask_offset.restype = [C.c_int, C.c_int, C.c_int], C.c_int64
    lib.ymi_post_decode_view.argtypes, lib.ymi_post_decode_view.restype = [C.POINTER(PostDesc), C.POINTER(PostView), C.c_void_p], C.c_int
    for f in (lib.ymi_post_begin, lib.ymi_post_finish, lib.ymi_postprocess):
        f.argtypes, f.restype = [C.POINTER(PostDesc), C.c_void_p], C.c_int
    out = dict(boxes=torch.full((n, k, 4), GUARD), scores=torch.full((n, k), GUARD), labels=torch.full((n, k), int(GUARD), dtype=torch.int64),
               count=torch.full((n,), int(GUARD), dtype=torch.int32), status=torch.full((8,), int(GUARD), dtype=torch.int32),
               ws=torch.full((int(lib.ymi_postprocess_ws_bytes(n, total, cap)),), 0x7f, dtype=torch.uint8))
    if flags & POST_CLASS_FILTER:
        off = int(lib.ymi_post_class_mask_offset(n, total, cap))
        out["ws"][off: off + 512] = torch.from_numpy(mask_words(classes).view(np.uint8).copy())
    out = {key: t.to(device) for key, t in out.items()}
    d = PostDesc()
    keep = []
    if plain:
        v, = views
        logits = nhwc_logits(v["heads"], nc, device)
        keep.append(logits)
        for i, ho in enumerate(v["heads"]):
            d.lh[i], d.lw[i], d.stride[i] = ho.shape[2], ho.shape[3], float(strides[i])
            d.logits[i], d.lcstride[i] = logits[i].data_ptr(), logits[i].shape[3]
            for j in range(6):
                d.anchors[i][j] = float(anchors[i][j])
        d.num_levels = len(v["heads"])
    else:
        d.num_levels, d.lh[0], d.lw[0] = 1, 1, total // 3
    d.n, d.num_classes = n, nc
    d.score_thresh, d.nms_thresh, d.detections_per_img = thr, nms, k
    d.out_boxes, d.out_scores, d.out_labels, d.out_count = out["boxes"].data_ptr(), out["scores"].data_ptr(), out["labels"].data_ptr(), out["count"].data_ptr()
    d.status, d.ws, d.ws_bytes, d.cand_cap, d.flags = out["status"].data_ptr(), out["ws"].data_ptr(), out["ws"].numel(), cap, flags

    def ok(rc):
        if rc != 0:
            err = getattr(lib, "sim_last_error", None) or lib.ymi_last_error
            err.restype = C.c_char_p
            raise AssertionError(err().decode())

    if plain:
        ok(lib.ymi_postprocess(C.byref(d), stream))
    else:
        ok(lib.ymi_post_begin(C.byref(d), stream))
        for v in views:
            logits = nhwc_logits(v["heads"], nc, device)
            keep.append(logits)
            pv = PostView()
            for i, ho in enumerate(v["heads"]):
                pv.logits[i], pv.lh[i], pv.lw[i], pv.lcstride[i], pv.stride[i] = logits[i].data_ptr(), ho.shape[2], ho.shape[3], logits[i].shape[3], float(strides[i])
                for j in range(6):
                    pv.anchors[i][j] = float(anchors[i][j])
            pv.num_levels, pv.skip_mask, pv.anchor_base, pv.scale, pv.flip_w = len(v["heads"]), v.get("skip", 0), v.get("base", 0), v.get("scale", 1.0), v.get("flip_w", 0)
            ok(lib.ymi_post_decode_view(C.byref(d), C.byref(pv), stream))
        ok(lib.ymi_post_finish(C.byref(d), stream))
    if device != "cpu":
        torch.cuda.synchronize()
    return {key: t.cpu() for key, t in out.items() if key != "ws"}


def tta_views(view_heads, canvas_w):
    """the three views of _forward_augment for run_views: skip masks and anchor bases of `layout`, scales and the mirror of the second view"""
    lay, total = layout([[(ho.shape[2], ho.shape[3]) for ho in hv] for hv in view_heads])
    return [dict(heads=hv, skip=lay[v][0], base=lay[v][1], scale=SCALES[v], flip_w=canvas_w if FLIPS[v] else 0) for v, hv in enumerate(view_heads)], total


def descale32(boxes, scale, flip_w):
    """the header's formulas in numpy float32, operation for operation: y' = y / s; x' = x / s, or x1' = W - x2 / s, x2' = W - x1 / s"""
    b = boxes.astype(F32)
    s = F32(scale)
    x1, y1, x2, y2 = (b[:, i] / s for i in range(4))
    if flip_w:
        x1, x2 = F32(flip_w) - x2, F32(flip_w) - x1
    return np.stack([x1, y1, x2, y2], 1).astype(F32)


def rows(out, i):
    c = int(out["count"][i])
    return out["boxes"][i, :c].numpy(), out["scores"][i, :c].numpy(), out["labels"][i, :c].numpy()


def expected_union(lib, view_heads, canvas_w, n, nc, strides, anchors, thr, k, cap, flags=0, classes=None, device="cpu"):
    """per image (boxes, scores, labels) of ALL candidates of the three views in the order the sort must give them: every view's kept levels through the library's own scale-1
    decode (ymi_postprocess with nms_thresh 1.0: nothing is suppressed, rank order = score descending, ties by anchor then class), boxes transformed by descale32,
    views concatenated in order, then a STABLE sort by score -- view-major, then anchor, then class among equal scores: the order of torch.cat(y, 1)"""
    views, _ = tta_views(view_heads, canvas_w)
    per_view = []
    for v in views:
        kept = [l for l in range(len(v["heads"])) if not (v["skip"] >> l) & 1]
        sub = dict(heads=[v["heads"][l] for l in kept])
        o = run_views(lib, [sub], n, nc, [strides[l] for l in kept], [anchors[l] for l in kept], thr, 1.0, k, cap, flags & ~POST_AGNOSTIC, classes, device, plain=True)
        assert int(o["status"][1]) == 0
        per_view.append(o)
    res = []
    for i in range(n):
        bs, ss, ls = [], [], []
        for v, o in zip(views, per_view):
            b, s, lab = rows(o, i)
            bs.append(descale32(b, v["scale"], v["flip_w"])), ss.append(s), ls.append(lab)
        b, s, lab = np.concatenate(bs), np.concatenate(ss), np.concatenate(ls)
        order = np.argsort(-s, kind="stable")
        res.append((b[order], s[order], lab[order]))
    return res


# ---- the whole post-process against the oracle ------------------------------------------------------------------------------------------------------------------------
def oracle_union(view_heads, canvas_w, strides, anchors):
    """O.decode per view -> _descale_pred in float64 (yolo.py:191-196: xywh / scale, x = W - x for the mirrored view) -> the concatenation without the tails
    (yolo.py:199-208).  -> (xywh float64 (n, A, 4), objectness and class confidences fp32 (n, A, 1 + nc)): the scores stay the oracle's fp32 values"""
    from oracle import yolov5_oracle as O
    lay, total = layout([[(ho.shape[2], ho.shape[3]) for ho in hv] for hv in view_heads])
    boxes, conf = [], []
    for v, hv in enumerate(view_heads):
        kept = [l for l in range(len(hv)) if not (lay[v][0] >> l) & 1]
        p = O.decode([hv[l] for l in kept], [strides[l] for l in kept], [anchors[l] for l in kept])
        b = p[..., :4].double() / SCALES[v]
        if FLIPS[v]:
            b[..., 0] = canvas_w - b[..., 0]
        boxes.append(b), conf.append(p[..., 4:])
    boxes, conf = torch.cat(boxes, 1), torch.cat(conf, 1)
    assert boxes.shape[1] == total
    return boxes, conf


def union_candidates(xywh, conf, thr, best=False, classes=None):
    """per image (boxes float64 xyxy, scores fp32, labels) in RANK order (score descending, ties in candidate order: view, anchor, class) -- the threshold, best-class and
    class-filter rules of tests/_merge_cases.candidates on the oracle's fp32 scores"""
    out = []
    for b4, c in zip(xywh, conf):
        scores = c[:, 1:] * c[:, 0:1]
        nc = scores.shape[1]
        allowed = torch.ones(nc, dtype=torch.bool) if classes is None else torch.zeros(nc, dtype=torch.bool)
        if classes is not None and len(classes):
            allowed[torch.tensor(sorted(classes), dtype=torch.long)] = True
        cx, cy, w, h = b4[:, 0], b4[:, 1], b4[:, 2], b4[:, 3]
        boxes = torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)
        if best:
            s, lab = scores.max(1)
            idx = torch.where(s > thr)[0]
            s, lab = s[idx], lab[idx]
        else:
            idx, lab = torch.where(scores > thr)
            s = scores[idx, lab]
        sel = allowed[lab]
        b, s, lab = boxes[idx][sel], s[sel], lab[sel]
        order = torch.sort(s, descending=True, stable=True)[1]
        out.append((b[order].numpy(), s[order].numpy(), lab[order].numpy()))
    return out


def oracle_reference(xywh, conf, thr, nms, k, best=False, agnostic=False, classes=None, merge=False, margin=1e-4):
    """the candidates above, the oracle's NMS, top-k and -- merge -- the float64 merge of tests/_merge_cases.merge_reference; per image dict(boxes float64, scores, labels).
    Asserts that no pair the NMS decides on (same label, or any under agnostic) has an IoU within `margin` of the threshold."""
    import _merge_cases as M
    cands = union_candidates(xywh, conf, thr, best, classes)
    for b, s, lab in cands:
        for i in range(len(s)):
            iou = M.iou64(b[i], b)
            close = np.abs(iou - nms) < margin
            if not agnostic:
                close &= lab == lab[i]
            assert not close.any(), f"a pair IoU within {margin} of the threshold: {iou[close]}"
    return M.merge_reference(cands, nms, k, agnostic, merge), cands


def assert_equals_reference(out, ref, what=""):
    """labels and order exact; scores and boxes with the tolerances of tests/test_e2e_gpu.py::test_postprocess_exact_given_oracle_logits; slots past the counts untouched"""
    for i, r in enumerate(ref):
        c = int(out["count"][i])
        assert c == len(r["scores"]), (what, i, c, len(r["scores"]))
        np.testing.assert_array_equal(out["labels"][i, :c].numpy(), r["labels"], err_msg=f"{what} image {i}")
        np.testing.assert_allclose(out["scores"][i, :c].numpy(), r["scores"], rtol=1e-5, atol=1e-6, err_msg=f"{what} image {i}")
        np.testing.assert_allclose(out["boxes"][i, :c].numpy(), r["boxes"], rtol=1e-5, atol=2e-3, err_msg=f"{what} image {i}")
        assert (out["scores"][i, c:] == GUARD).all() and (out["boxes"][i, c:] == GUARD).all(), f"{what} image {i}: slots past the count were written"


CANVAS = (128, 160)
WHOLE_RUNS = (   # (nc, thr, nms, k, best, agnostic, classes, merge)
    (2, 0.3, 0.45, 300, False, False, None, False),
    (2, 0.3, 0.5, 300, False, True, None, False),    # (agnostic at 0.45: one pair of the union has IoU 0.44992, inside the margin that oracle_reference asserts)
    (2, 0.3, 0.45, 300, False, False, None, True),
    (80, 0.3, 0.45, 300, False, False, (0, 3, 17, 41, 79), False),
    (2, 0.3, 0.45, 300, True, False, None, False),
)


def whole_case(nc, n=2):
    """random heads of the three views of a 128 x 160 canvas (view canvases 128 x 160, 128 x 160, 96 x 128)"""
    from oracle import yolov5_oracle as O
    strides, anchors = O.anchors_for(3)
    shapes = view_shapes(*CANVAS, strides)
    view_heads = [_post_cases.post_heads(nc, sh, n=n, seed=31 + 7 * v) for v, sh in enumerate(shapes)]
    return view_heads, strides, anchors


def run_flags(best, agnostic, classes, merge):
    return (POST_BEST_CLASS if best else 0) | (POST_AGNOSTIC if agnostic else 0) | (POST_CLASS_FILTER if classes is not None else 0) | (POST_MERGE if merge else 0)
