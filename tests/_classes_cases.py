"""Shared by tests/test_class_filter.py (CPU: host logic, the oracle's own non-vacuity figures, the simulator) and tests/test_class_filter_gpu.py (the real kernels): class
sets, the reference of the CLASS FILTER (include/yolort_amd.h YMI_POST_CLASS_FILTER; Python `classes=[...]`; ultralytics' non_max_suppression(..., classes=...),
yolort/v5/utils/general.py:585-587) and the GPU drivers that carry a class set through the host redo protocol.

The reference is the oracle's decode, then the filter as the header states it, then O.batched_nms (labels zeroed for the call when agnostic), then the first k:
  multi-label  an (anchor, class) pair is a candidate iff cls * obj > thr (strict) and the class is in the set;
  best-class   (conf, j) = scores.max(1) over ALL classes -- torch's first maximal index --, the anchor is a candidate iff conf > thr and j is in the set.
`order="after"` (NMS first, filter the survivors) and `reading="allowed-argmax"` (the maximum over the allowed classes only) are the two MISREADINGS the tests show to
differ from it; nothing but the oracle enters either."""
import functools

import numpy as np
import torch

import _agnostic_cases as A
import _head_cases as H

POST_CLASS_FILTER, POST_AGNOSTIC, POST_BEST_CLASS, POST_EXACT_FULL = 8, 4, 2, 1   # include/yolort_amd.h (restated so that a missing constant fails a test, not the collection)
MASK_WORDS = 128

# nc = 80.  Channel = class + 5, the head's register layout has 32-row sub-tiles: set A holds exactly one side of either boundary (27 | 26: channels 32 | 31, 58 | 59:
# channels 63 | 64), the first and the last class, and classes of both lane halves ((class + 5) % 8 < 4: 27, 31, 64, 7 ...; >= 4: 0, 2, 58, 79)
SET_A = (0, 2, 5, 7, 27, 31, 58, 64, 79)
SET_B = tuple(c for c in range(80) if c not in SET_A)
RUNS = ((0.3, 300), (0.05, 7), (0.05, 300))


def set_a(nc):
    """set A for a class count: as it is at 80, (1,) at 2, reduced modulo nc below 80"""
    if nc == 80:
        return SET_A
    if nc == 2:
        return (1,)
    return tuple(sorted({c % nc for c in SET_A}))


def mask_words(classes):
    w = np.zeros(MASK_WORDS, np.uint32)
    for c in classes:
        w[c >> 5] |= np.uint32(1 << (c & 31))
    return w


def _oracle():
    from oracle import yolov5_oracle as O
    return O


def filtered_reference(pred, thr, nms, k, best, agnostic, classes, order="before", reading="stated"):
    """-> [{scores, labels, boxes}] per image.  classes None = no filter."""
    O = _oracle()
    dets = []
    for p in pred:
        scores = p[:, 5:] * p[:, 4:5]
        nc = scores.shape[1]
        allowed = torch.ones(nc, dtype=torch.bool) if classes is None else torch.zeros(nc, dtype=torch.bool)
        if classes is not None and len(classes):
            allowed[torch.tensor(sorted(classes), dtype=torch.long)] = True
        cx, cy, w, h = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
        boxes = torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)
        if best:
            if reading == "allowed-argmax":   # the misreading: the best ALLOWED class
                conf, j = torch.where(allowed[None, :], scores, torch.full_like(scores, -1.0)).max(1)
            else:
                conf, j = scores.max(1)
            keep = conf > thr
            b, s, lab = boxes[keep], conf[keep], j[keep]
        else:
            inds, lab = torch.where(scores > thr)
            b, s = boxes[inds], scores[inds, lab]
        if order == "before":
            sel = allowed[lab]
            b, s, lab = b[sel], s[sel], lab[sel]
        kept = O.batched_nms(b, s, torch.zeros_like(lab) if agnostic else lab, nms)
        if order == "after":
            kept = kept[allowed[lab[kept]]]
        kept = kept[:k]
        dets.append({"scores": s[kept], "labels": lab[kept], "boxes": b[kept]})
    return dets


@functools.lru_cache(maxsize=None)
def full_ref(nc, sim, thr, best, agnostic, classes, order="before", reading="stated"):
    """the un-truncated survivors of A.post_inputs(nc, "full", sim) (the top-k cut is a slice of them); computed once, left unchanged"""
    return filtered_reference(A.post_inputs(nc, "full", sim)[3], thr, 0.45, 1 << 30, best, agnostic, classes, order, reading)


def candidate_counts(pred, thr, best, classes):
    """per image: what status[4] counts -- passing pairs of allowed classes / passing anchors whose best class is allowed"""
    out = []
    for p in pred:
        scores = p[:, 5:] * p[:, 4:5]
        allowed = torch.zeros(scores.shape[1], dtype=torch.bool)
        if classes is None:
            allowed[:] = True
        elif len(classes):
            allowed[torch.tensor(sorted(classes), dtype=torch.long)] = True
        if best:
            conf, j = scores.max(1)
            out.append(int(((conf > thr) & allowed[j]).sum()))
        else:
            out.append(int(((scores > thr) & allowed[None, :]).sum()))
    return out


# ---- the real kernels through the plan, under the host protocol of yolort_amd/ops.py: the mode flags AND the class set stay in every redo ----
def gpu_post(dev, heads, strides, anchors, nc, thr, k, cap, flags, classes, fill=-3.0, one_pass=False):
    """_agnostic_cases.gpu_post with a class set (None: no filter): every pass builds a fresh plan, whose workspace gets the mask again"""
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
        pb = plan.postprocess(views, strides, anchors, nc, thr, 0.45, k, cap, flags=flags, classes=classes)
        pb.boxes.fill_(fill), pb.scores.fill_(fill), pb.labels.fill_(int(fill)), pb.status_count.fill_(int(fill)), pb.slab.fill_(fill)
        plan.run()
        st = pb.status.cpu().tolist()
        passes.append(st)
        assert len(passes) <= 6, passes
        if st[1] == 0 or one_pass:
            return dict(count=pb.count.cpu(), labels=pb.labels.cpu(), scores=pb.scores.cpu(), boxes=pb.boxes.cpu(), slab=pb.slab.cpu(), passes=passes, cap=cap)
        if not st[1] & 1:
            flags |= POST_EXACT_FULL
            continue
        need = max(st[0], st[3] * n)
        cap = max(int(need * 1.25) + 1024, 2 * cap)
        cap = n * (1 << ((cap + n - 1) // n - 1).bit_length())


def _gpu_head_pass(dev, case, head, mode, cap, flags, fill, classes):
    """_head_cases._gpu_head_pass with a class set"""
    from yolort_amd.engine import Plan, View
    n, nc, kk, dtype = case["n"], case["nc"], case["nc"] + 5, case["dtype"]
    plan = Plan(dev, dtype)
    args = (case["strides"], case["anchors"], nc, case["thr"], case["nms"], case["k"], cap)
    if mode == "unfused":
        views = []
        for lg in case["logits"]:
            h, w, cs = lg.shape[2], lg.shape[3], (3 * kk + 3) // 4 * 4
            t = torch.zeros(n, h, w, cs, device=dev, dtype=torch.float32)
            t[..., : 3 * kk] = lg.to(dev).permute(0, 2, 3, 1, 4).reshape(n, h, w, 3 * kk)
            views.append(View(t.view(-1), 0, n, h, w, 3 * kk, cs))
        pb = plan.postprocess(views, *args, flags=flags, classes=classes)
    else:
        xs, pcs = [], []
        for i, x in enumerate(case["x"]):
            _, h, w, cin = x.shape
            if case["wide"]:
                buf = plan.alloc(n, h, w, cin + 2 * H.WIDE_PAD)
                buf.as_tensor().fill_(H.WIDE_VALUE)
                v = buf.slice_c(H.WIDE_PAD, cin)
            else:
                v = plan.alloc(n, h, w, cin)
            v.as_tensor().copy_(torch.from_numpy(x).to(dev))
            xs.append(v)
            pcs.append(head.packed_anchor_major(i, dtype, dev, cin))
        pb, d = plan.post_desc(case["shapes"], n, *args, flags=flags, classes=classes)
        plan.post_begin(d)
        if mode == "group":
            plan.head_decode_group(xs, pcs, d)
        else:
            for i in range(len(xs)):
                plan.head_decode(xs[i], pcs[i], d, i)
        plan.post_finish(d, pb.total_anchors)
    pb.boxes.fill_(fill), pb.scores.fill_(fill), pb.labels.fill_(int(fill)), pb.status_count.fill_(int(fill))
    plan.run()
    torch.cuda.synchronize()
    pb.plan = plan
    return pb


def gpu_head(dev, case, mode, classes, flags=0, fill=-3.0):
    """_head_cases.gpu_head with a class set kept across the redos"""
    head = None if mode == "unfused" else H.make_head(case)
    n, cap, passes = case["n"], case["cand_cap"], []
    while True:
        pb = _gpu_head_pass(dev, case, head, mode, cap, flags, fill, classes)
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


@functools.lru_cache(maxsize=None)
def head_filtered_reference(name, best=False):
    """head_reference of a case of _head_cases, filtered by the case's set A"""
    c = H.head_case(name)
    return filtered_reference(c["pred"], c["thr"], c["nms"], c["k"], best, False, set_a(c["nc"]))
