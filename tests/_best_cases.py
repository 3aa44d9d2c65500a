"""Shared by tests/test_best_class.py (CPU: host logic, the simulator, the sigmoid sweep) and tests/test_best_class_gpu.py (the real kernels): the reference of the BEST-CLASS
post-process mode (include/yolort_amd.h YMI_POST_BEST_CLASS: one label per anchor, the contract of ultralytics' non_max_suppression(..., multi_label=False),
yolort/v5/utils/general.py:572-583), and small inputs with EXACT logits (the rules of tests/_head_cases.py: one 1.0 per 32-channel block, weights exact in fp16 and bf16,
fp32 bias), each named for the mistake it catches.

The reference restates general.py:572-583 on the oracle's pieces: scores = cls * obj, (conf, j) = scores.max(1) -- torch's first maximal index --, keep conf > thr, boxes as
O.postprocess builds them, O.batched_nms, the first k.  The new cases live on n = 2, one 5 x 7 level plus one 1 x 3 level: 35 pixels an image, so the second 32-pixel wave
spans both images and the last wave of either level is partial."""
import functools

import numpy as np
import torch

import _head_cases as H

F32 = np.float32
POST_BEST_CLASS = 2   # include/yolort_amd.h YMI_POST_BEST_CLASS (yolort_amd._lib.POST_BEST_CLASS; restated so that a missing constant fails a test, not the collection)

# the exact cases of tests/_head_cases.py that are run in best-class mode
EXISTING = tuple(f"nc{nc}-float16" for nc in (27, 28, 59, 60, 91, 92, 123)) + ("nc28-bfloat16", "dense", "levels-1", "levels-2", "levels-4", "tie-half", "tie-below-half",
                                                                               "tie-quarter", "tie-below-quarter", "palette-mixed", "thr-zero", "thr-negative", "global-sink", "nms")
# The palette of these three (objectness 0.5, class scores 0.5 / 0.25 / 1e-9 against a threshold of 0.5, the float below it, 0.25) lets at most ONE class of an anchor
# pass: the two modes agree there by design (what they check in this mode is the tie at the threshold).  Every other case must tell the modes apart.
ONE_PASSING_CLASS = ("tie-half", "tie-below-half", "tie-quarter")

G2 = dict(n=2, shapes=[(5, 7), (1, 3)], chans=[32, 32])


def best_postprocess(pred, thr, nms, k):
    """general.py:572-583 (multi_label=False) on the oracle's decode `pred` (n, anchors, 5 + nc) -> [{scores, labels, boxes}] per image"""
    from oracle import yolov5_oracle as O
    dets = []
    for p in pred:
        scores = p[:, 5:] * p[:, 4:5]
        conf, j = scores.max(1)
        keep = conf > thr
        cx, cy, w, h = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
        boxes = torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)
        b, s, lab = boxes[keep], conf[keep], j[keep]
        kept = O.batched_nms(b, s, lab, nms)[:k]
        dets.append({"scores": s[kept], "labels": lab[kept], "boxes": b[kept]})
    return dets


# ---- the new cases: name -> (nc, thr, dtype, kinds(nc) -> (objectness (3, 32), classes (3, nc, 32)), box logit or None, exact scores, expected records or None) ----
def _shift(a):
    """anchor q sees the kinds rotated by q: the three anchors of a pixel differ"""
    return np.stack([np.roll(a, q, axis=-1) for q in range(3)])


def _k_equal_products(nc):
    # objectness 0.5; sigmoid(20) and sigmoid(24) are both exactly 1.0: the products of logits 20 and 24 are EQUAL (0.5), the label is the lowest index among them -- not
    # the index of the largest logit (kinds 0 mod 3: label 1, the 24 sits at 2; kinds 1 mod 3: label 0, the 24 comes first); kinds 2 mod 3: objectness fails
    cls = np.zeros((nc, 32), F32)
    obj = np.zeros(32, F32)
    for kd in range(32):
        cls[:, kd] = [(0, 20, 24, 20, -20), (24, 0, 20, 20, -20), (0, 20, 24, 20, -20)][kd % 3]
        obj[kd] = -20.0 if kd % 3 == 2 else 0.0
    return _shift(obj), _shift(cls)


def _k_equal_logits(nc):
    # nc = 60 (K = 65, three 32-row sub-tiles).  Class 1 is row 6 (sub-tile 0, upper lane half), class 40 row 45 (sub-tile 1), class 2 row 7 (upper half, last register of
    # its group), class 3 row 8 (lower half, next group), class 59 row 64 (sub-tile 2), class 0 row 5: equal logits at both, the lower index has to win in the register
    # pass, in the cross-half exchange and across sub-tiles
    cls = np.full((nc, 32), -6.0, F32)
    for kd in range(32):
        a, b = [(1, 40), (2, 3), (59, 0), (40, 41)][kd % 4]
        cls[a, kd] = cls[b, kd] = 3.0
    return _shift(np.full(32, 2.0, F32)), _shift(cls)


def _k_padding(nc):
    # every real class logit is negative, the padding rows of the anchor (logit 0: sigmoid 0.5) would beat them all; the best real class moves with the kind
    cls = np.zeros((nc, 32), F32)
    for kd in range(32):
        cls[:, kd] = -2.0 - 0.25 * ((np.arange(nc) + kd) % 5)
        cls[(7 * kd + 1) % nc, kd] = -1.0
    return _shift(np.full(32, 6.0, F32)), _shift(cls)


def _k_box_rows(nc):
    # box logits 1.5 and objectness logit 6 lie above every class logit: rows 0 ... 4 must not take part in the maximum (nor raise the cut above every class)
    cls = np.zeros((nc, 32), F32)
    for kd in range(32):
        cls[:, kd] = np.roll(np.array([1.0, 0.5, -1.0], F32), kd % 3)
    return _shift(np.full(32, 6.0, F32)), _shift(cls)


def _k_first_last(nc):
    # the best class in the last real row (c = K - 1) and in the first (c = 5)
    cls = np.full((nc, 32), -4.0, F32)
    for kd in range(32):
        cls[nc - 1 if kd % 2 == 0 else 0, kd] = 2.0
        cls[nc // 2, kd] = 1.5
    return _shift(np.full(32, 3.0, F32)), _shift(cls)


def _k_conf_at_thr(nc):
    # objectness 0.5, best class 1.0: conf is exactly 0.5 (kinds 0 mod 3), exactly 0.25 (1 mod 3), or the objectness fails
    cls = np.zeros((nc, 32), F32)
    obj = np.zeros(32, F32)
    for kd in range(32):
        cls[:, kd] = [(0, 20, -20), (-20, 0, 0), (20, 20, 20)][kd % 3]
        obj[kd] = -20.0 if kd % 3 == 2 else 0.0
    return _shift(obj), _shift(cls)


def _k_obj_passes_best_fails(nc):
    # objectness 0.88 passes the threshold 0.3; kinds 0 mod 2: every product is 0.042 (nothing), kinds 1 mod 2: one class at logit 2 (0.78)
    cls = np.full((nc, 32), -3.0, F32)
    for kd in range(1, 32, 2):
        cls[kd % nc, kd] = 2.0
    return _shift(np.full(32, 2.0, F32)), _shift(cls)


def _k_one_class(nc):
    rng = np.random.default_rng(11)
    return rng.integers(-4, 3, (3, 32)).astype(F32), rng.choice(np.array([-6.0, 0.0, 1.0, 2.0, 3.0, 4.0], F32), (3, nc, 32))


NEW_SPECS = {
    "equal-products": dict(nc=5, thr=0.3, kinds=_k_equal_products, exact=(0.5,)),
    "equal-logits-nc60": dict(nc=60, thr=0.3, kinds=_k_equal_logits),
    "padding-nc3": dict(nc=3, thr=0.05, kinds=_k_padding),
    "padding-nc28": dict(nc=28, thr=0.05, kinds=_k_padding),
    "padding-nc60": dict(nc=60, thr=0.05, kinds=_k_padding),
    "padding-nc92-bfloat16": dict(nc=92, thr=0.05, kinds=_k_padding, dtype="bfloat16"),
    "box-rows": dict(nc=3, thr=0.3, kinds=_k_box_rows, box=1.5),
    "first-last-row-nc28": dict(nc=28, thr=0.3, kinds=_k_first_last),
    "first-last-row-nc27": dict(nc=27, thr=0.3, kinds=_k_first_last),
    "conf-equals-thr": dict(nc=3, thr=H.HALF, kinds=_k_conf_at_thr, exact=(0.25, 0.5), tie=True, expect=0),
    "conf-above-thr": dict(nc=3, thr=H.BELOW_HALF, kinds=_k_conf_at_thr, exact=(0.25, 0.5)),   # one record per anchor of a kind 0 mod 3 (counted from the reference)
    "objectness-passes-best-fails": dict(nc=4, thr=0.3, kinds=_k_obj_passes_best_fails),
    "one-class": dict(nc=1, thr=0.3, kinds=_k_one_class),
}
NEW_CASES = tuple(NEW_SPECS)
NA3_CASES = ("tie-below-quarter", "equal-products", "equal-logits-nc60", "padding-nc3", "padding-nc28", "padding-nc60", "padding-nc92-bfloat16", "nc27-float16",
             "nc59-float16", "nc91-float16", "nc123-float16")   # the YOLORT_AMD_HEAD_SPLIT=0 child: the ties, the paddings, one class count per TNA
SIM_HEAD_CASES = ("equal-products", "padding-nc3", "box-rows", "equal-logits-nc60", "padding-nc60")   # TNA 1 (nc = 3, 5) and TNA 3 (nc = 60)


@functools.lru_cache(maxsize=None)
def best_case(name):
    """a case in the format of _head_cases.head_case (what _gpu_head_pass and make_head read); the existing cases are passed through.  Cached and left unchanged."""
    if name in H.SPECS:
        return H.head_case(name)
    from oracle import yolov5_oracle as O
    spec = NEW_SPECS[name]
    n, nc, shapes, chans = G2["n"], spec["nc"], G2["shapes"], G2["chans"]
    kk = nc + 5
    rng = np.random.default_rng([7, sum(ord(ch) * (i + 1) for i, ch in enumerate(name))])
    strides, anchors = O.anchors_for(3)
    strides, anchors = list(strides[:2]), [list(map(float, a)) for a in anchors[:2]]
    xs, ws, bs, logits = [], [], [], []
    for lvl, ((h, w), cin) in enumerate(zip(shapes, chans)):
        m_all = n * h * w
        obj, cls = spec["kinds"](nc)
        wt = np.zeros((3, kk, cin), F32)
        wt[:, :4] = (rng.integers(-96, 97, (3, 4, 32)) * 2.0 ** -6).astype(F32) if spec.get("box") is None else F32(spec["box"])
        wt[:, 4], wt[:, 5:] = obj, cls
        bias = np.zeros((3, kk), F32)
        bias[:, :4] = (rng.integers(-256, 257, (3, 4)) * 2.0 ** -10).astype(F32) if spec.get("box") is None else 0.0
        kind = (np.arange(m_all) * 5 + 3 + 11 * lvl) % 32      # 5 is odd: the 70 pixels of level 0 meet every kind, the 6 of level 1 six different ones
        x = np.zeros((m_all, cin), F32)
        x[np.arange(m_all), kind] = 1.0
        w2 = wt.reshape(3 * kk, cin)
        tw = torch.from_numpy(w2)
        assert torch.equal(tw.half().float(), tw) and torch.equal(tw.bfloat16().float(), tw), f"{name}: a weight is not exact in fp16 and bf16"
        lg64 = x.astype(np.float64) @ w2.astype(np.float64).T + bias.reshape(-1).astype(np.float64)
        lg = lg64.astype(F32)
        assert (lg.astype(np.float64) == lg64).all()
        xs.append(x.reshape(n, h, w, cin))
        ws.append(w2)
        bs.append(bias.reshape(-1))
        logits.append(torch.from_numpy(lg.reshape(n, h, w, 3, kk)).permute(0, 3, 1, 2, 4).contiguous())
    thr = float(spec["thr"])
    pred = O.decode(logits, strides, anchors)
    cand = (pred[..., 5:] * pred[..., 4:5]) > thr
    total_anchors = sum(3 * h * w for h, w in shapes)
    return dict(name=name, dtype=getattr(torch, spec.get("dtype", "float16")), n=n, nc=nc, shapes=shapes, chans=chans, strides=strides, anchors=anchors, thr=thr, nms=1.0,
                k=(total_anchors + 64) // 64 * 64, cand_cap=n * 16384, wide=False, tie=bool(spec.get("tie", False)), guards=(), exact=tuple(spec.get("exact", ())),
                expect_candidates=spec.get("expect"), dense=[], design="best", x=xs, weight=ws, bias=bs, logits=logits, pred=pred, cand=cand,
                candidates_per_image=cand.sum((1, 2)).tolist())


@functools.lru_cache(maxsize=None)
def best_reference(name):
    c = best_case(name)
    return best_postprocess(c["pred"], c["thr"], c["nms"], c["k"])


def assert_best_case_is_not_vacuous(name):
    """from the ORACLE's decode alone: no best score other than a designed exact value lies within NEAR_REL of the threshold; a case with nc > 1 tells the two modes apart
    (some anchor has two passing classes, and the best-class reference differs from the multi-label one) unless it is one of ONE_PASSING_CLASS, where that is asserted to
    be impossible; the named mistake of a new case would change the result.  -> a line of figures to print"""
    from oracle import yolov5_oracle as O
    case, ref = best_case(name), best_reference(name)
    thr, nc, pred = F32(case["thr"]), case["nc"], case["pred"]
    scores = (pred[..., 5:] * pred[..., 4:5])
    conf, label = scores.max(-1)
    c = conf.numpy()
    designed = np.isin(c, np.array(case["exact"], F32))
    near = (np.abs(c.astype(np.float64) - float(thr)) <= H.NEAR_REL * abs(float(thr))) & ~designed
    assert not near.any(), f"{name}: best scores within {H.NEAR_REL} (relative) of the threshold {thr!r}: {c[near][:5]}"
    ties = c == thr
    assert (designed | ~ties).all() and (name in H.SPECS or not case["tie"] or ties.any()), f"{name}: {int(ties.sum())} best scores equal the threshold"
    passing = (scores > float(thr)).sum(-1)
    two = bool((passing >= 2).any())
    multi = O.postprocess(pred, case["thr"], case["nms"], case["k"])
    differs = any(len(a["scores"]) != len(b["scores"]) or not torch.equal(a["labels"], b["labels"]) for a, b in zip(ref, multi))
    if name in H.SPECS and nc > 1:
        assert two == (name not in ONE_PASSING_CLASS), f"{name}: an anchor with two passing classes: {two}"
        assert differs == two, f"{name}: the best-class reference {'differs from' if differs else 'equals'} the multi-label one"
    n_ref = sum(len(r["scores"]) for r in ref)
    if case["nms"] >= 1.0 and n_ref < case["k"]:
        assert n_ref == int((conf > float(thr)).sum())
    if case["expect_candidates"] is not None and name in NEW_SPECS:
        assert n_ref == case["expect_candidates"], (name, n_ref)
    if name in NEW_SPECS:
        assert n_ref > 0 or case["expect_candidates"] == 0, f"{name}: no record at all"
        lg = torch.cat([l_.reshape(case["n"], -1, nc + 5) for l_ in case["logits"]], 1)   # (n, anchors, K) in the order of pred
        ok = conf > float(thr)
        if name == "equal-products":   # the largest LOGIT sits elsewhere than the label
            assert bool((lg[..., 5:].argmax(-1)[ok] != label[ok]).any())
        if name == "equal-logits-nc60":   # every pair of tied classes is met, the lower one is the label
            assert set(label[ok].tolist()) == {1, 2, 0, 40}
        if name.startswith("padding"):   # a padding row (logit 0, sigmoid 0.5) would beat the best real class of every anchor
            assert bool((lg[..., 5:] < 0).all()) and (nc + 5) % 32 != 0 and bool(ok.all())
        if name == "box-rows":
            assert bool((lg[..., :5].min(-1).values > lg[..., 5:].max(-1).values).all()) and bool(ok.all())
        if name.startswith("first-last-row"):
            assert set(label[ok].tolist()) == {0, nc - 1}
        if name == "conf-above-thr":
            assert 0 < n_ref == int((c == F32(0.5)).sum()) and bool(((c == F32(0.25)) & ~ok.numpy()).any())
        if name == "conf-equals-thr":
            assert int(ties.sum()) > 0
        if name == "objectness-passes-best-fails":
            assert bool(((pred[..., 4] > float(thr)) & ~ok).any()) and bool(ok.any())
        if name == "one-class":
            assert not differs and 0 < n_ref < conf.numel()
    return f"{name}: passing anchors {(conf > float(thr)).sum(-1).tolist()} of {conf.shape[1]}, multi-label candidates {case['candidates_per_image']}, two passing classes: {two}"


# ---- the real kernels through the C ABI, under the host protocol of yolort_amd/ops.py (the flag stays set in every redo) ----
def gpu_best(dev, case, mode, flags=POST_BEST_CLASS, fill=-3.0):
    head = None if mode == "unfused" else H.make_head(case)
    n, cap, passes = case["n"], case["cand_cap"], []
    while True:
        pb = H._gpu_head_pass(dev, case, head, mode, cap, flags, fill)
        st = pb.status.cpu().tolist()
        passes.append(st)
        assert len(passes) <= 6, passes
        if st[1] == 0:
            return dict(count=pb.count.cpu(), labels=pb.labels.cpu(), scores=pb.scores.cpu(), boxes=pb.boxes.cpu(), passes=passes, cap=cap)
        if not st[1] & 1:
            flags |= 1   # YMI_POST_EXACT_FULL
            continue
        need = max(st[0], st[3] * n)
        cap = max(int(need * 1.25) + 1024, 2 * cap)
        cap = n * (1 << ((cap + n - 1) // n - 1).bit_length())
