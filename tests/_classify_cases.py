"""Cases and float64 references of the second-stage classification (include/yolort_amd.h ymi_classify_head / ymi_second_stage_filter; ops.classify_head,
ops.second_stage_filter), written from the contract: mean over the pixels, matrix products, Hardswish, arg-max, a Python loop for the filter.  No machinery.

Error bound of a general case (`bound`), per logit, u = 2^-11 (fp16) or 2^-8 (bf16), v = 2^-24 (fp32), t = 2^-25 for fp16 (a subnormal's rounding), operands exact:
  pooled  p^ = round_dtype(fl32(sum) * fl32(1/hw)):  ep[k] = u |p[k]| + (hw + 2) v mean|x[.., k]| + t       (hw - 1 fp32 additions, 1/hw, the product; one rounding)
  stage   z^ = fp32 sum over K of exact products + bias:  ez[j] = sum_k ep[k] |w1[j][k]| + (K + 2) v (sum_k |p[k]| |w1[j][k]| + |b1[j]|)
  hidden  h^ = round_dtype(hardswish32(z^)), |hardswish'| <= 1.5:  eh[j] = 1.5 ez[j] + (u + 4 v)(|h[j]| + 1.5 ez[j]) + t
  logits  el[m] = sum_j eh[j] |w2[m][j]| + (N1 + 2) v (sum_j |h[j]| |w2[m][j]| + |b2[m]|);  one stage: el = ez.
It is a worst-case sum, yet tight enough that a dropped K step of a row fails it: the maps are uniform in [0, 1) (p ~ 0.5) and the weights uniform in +-0.25 (rms
0.144), so 64 dropped terms move a first-stage sum by about sqrt(64) * 0.5 * 0.144 = 0.58, while one-stage bounds are about K * u * 0.5 * 0.125: 0.008 (fp16) or
0.06 (bf16) at K = 256, 0.002 / 0.016 at K = 80.  Through a second stage a dropped hidden step moves a logit by about sqrt(64) * E|h| * 0.144 ~ 0.8 at N1 = 256, against
bounds of 0.33 .. 0.47 (fp16); the one case where the worst-case sum exceeds that is bf16 at K = N1 = 256 (2.6 .. 3.6: 256 terms of 2^-8 relative error each, twice) --
there the bf16 property is carried by the smaller shapes (n31_c40: one K step IS the row, bound 0.06 .. 0.10) and by the exact cases, where any dropped term is a wrong bit.
"""
import numpy as np
import torch

# (name, n, [(h, w, c, channel stride)], N1, N2 or None = one stage).  n around BM = 32; C = 8, 40, 256 and 72 (a multiple of 8, not of the K step 64 nor of an
# MFMA's 16); classes 1, 5, 33, 1000; a channel stride above c; two and four maps of unequal c; a hidden width that differs from C.
CASES = [
    ("n1_c8", 1, [(1, 1, 8, 8)], 8, 1),
    ("n31_c40", 31, [(2, 2, 40, 40)], 40, 5),
    ("n32_c72", 32, [(4, 4, 72, 72)], 72, 33),
    ("n33_c256", 33, [(2, 2, 256, 256)], 256, 1000),
    ("n67_stride", 67, [(1, 16, 40, 64)], 24, 5),
    ("n33_two_maps", 33, [(2, 2, 8, 8), (1, 1, 16, 24)], 5, None),
    ("n67_four_maps", 67, [(4, 4, 8, 8), (1, 2, 24, 24), (1, 1, 16, 32), (2, 2, 8, 8)], 33, None),
    ("n1_one_stage_1000", 1, [(1, 1, 256, 256)], 1000, None),
    ("n31_7x7", 31, [(7, 7, 40, 40)], 40, 33),          # general only: h * w is no power of two
    ("n33_1x20", 33, [(1, 20, 72, 80), (7, 7, 8, 8)], 5, None),
]
EXACT = [c for c in CASES if all((h * w) & (h * w - 1) == 0 for h, w, _, _ in c[2])]
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
hardswish = lambda x: x * np.minimum(np.maximum(x + 3.0, 0.0), 6.0) / 6.0   # noqa: E731


def head_ref(maps, w1, b1, w2=None, b2=None):
    """float64: maps [(n, h, w, c)] -> logits (n, N_last)"""
    p = np.concatenate([m.reshape(m.shape[0], -1, m.shape[3]).mean(1) for m in maps], 1)
    z = p @ w1.T + b1
    return z if w2 is None else hardswish(z) @ w2.T + b2


def bound(maps, w1, b1, w2, b2, dtype):
    u, v, t = UNIT[dtype], 2.0 ** -24, (2.0 ** -25 if dtype == torch.float16 else 0.0)
    flat = [m.reshape(m.shape[0], -1, m.shape[3]) for m in maps]
    p = np.concatenate([f.mean(1) for f in flat], 1)
    ep = np.concatenate([u * np.abs(f.mean(1)) + (f.shape[1] + 2) * v * np.abs(f).mean(1) + t for f in flat], 1)
    ez = ep @ np.abs(w1).T + (p.shape[1] + 2) * v * (np.abs(p) @ np.abs(w1).T + np.abs(b1))
    if w2 is None:
        return ez
    h = np.abs(hardswish(p @ w1.T + b1))
    eh = 1.5 * ez + (u + 4 * v) * (h + 1.5 * ez) + t
    return eh @ np.abs(w2).T + (w1.shape[0] + 2) * v * (h @ np.abs(w2).T + np.abs(b2))


def general_case(case, seed=0):
    """random operands, float64 holding values that are exact in fp16 AND bf16 (multiples of 2^-7 below 1): maps in [0, 1), weights in +-0.25, biases in +-0.5"""
    _, n, maps, n1, n2 = case
    g = np.random.default_rng(seed)
    ms = [g.integers(0, 128, (n, h, w, c)) / 128.0 for h, w, c, _ in maps]
    k = sum(c for _, _, c, _ in maps)
    w1, b1 = g.integers(-32, 33, (n1, k)) / 128.0, g.integers(-64, 65, n1) / 128.0
    w2, b2 = (None, None) if n2 is None else (g.integers(-32, 33, (n2, n1)) / 128.0, g.integers(-64, 65, n2) / 128.0)
    return ms, w1, b1, w2, b2


def exact_case(case):
    """Operands whose every intermediate is an integer that fp16 and bf16 hold: pooled p[r][k] = A[r] + c[k] (A distinct per row in 4 .. 70, c distinct per channel in
    -128 .. 127), pixel q adds d[q] with sum_q d = 0; w1 small integers whose row sums are +-1 / +-2, the channel part sum_k c[k] w1[j][k] taken out by the (fp32) bias,
    so z[r][j] = A[r] * rowsum[j] + sign * (j % 8): an integer of magnitude 4 .. 147, and Hardswish returns z or 0.  A permuted, dropped or repeated channel breaks
    the cancellation; a permuted row changes A."""
    _, n, maps, n1, n2 = case
    g = np.random.default_rng(7)
    k = sum(c for _, _, c, _ in maps)
    cvals = g.permutation(256)[:k] - 128.0
    p = (4.0 + np.arange(n))[:, None] + cvals[None, :]
    ms, k0 = [], 0
    for h, w, c, _ in maps:
        q = np.arange(h * w)
        d = np.where(q % 2 == 0, q // 2 + 1.0, -(q // 2 + 1.0)) if h * w > 1 else np.zeros(1)
        ms.append((p[:, None, k0:k0 + c] + d[None, :, None]).reshape(n, h, w, c))
        k0 += c
    w1 = g.integers(-3, 4, (n1, k)).astype(np.float64)
    rowsum = np.array([1.0, -1.0, 2.0, -2.0])[np.arange(n1) % 4]
    w1[:, 0] += rowsum - w1.sum(1)
    assert np.abs(w1).max() <= 256                      # integers bf16 holds (the seed is fixed: the largest correction is 3.5 sigma of sqrt(256 * 4))
    b1 = -(w1 @ cvals) + np.sign(rowsum) * (np.arange(n1) % 8)
    w2, b2 = (None, None) if n2 is None else (g.integers(-4, 5, (n2, n1)).astype(np.float64), g.integers(-9, 10, n2).astype(np.float64))
    return ms, w1, b1, w2, b2


def filter_ref(boxes, scores, labels, counts, logits, total, class_map=None):
    n, k = scores.shape
    ob, os_, ol, oc, cls2 = np.zeros_like(boxes), np.zeros_like(scores), np.zeros_like(labels), np.zeros(n, np.int32), np.full((n, k), -1, np.int32)
    clamped = [min(max(int(c), 0), k) for c in counts]
    cap, row = logits.shape[0], 0
    limit = min(max(int(total[0]), 0), cap)
    status = (1 if any(c < 0 or c > k for c in counts) else 0) | (2 if int(total[0]) != min(sum(clamped), cap) else 0) | (4 if sum(clamped) > cap else 0)
    for i in range(n):
        for j in range(clamped[i]):
            if row < limit:
                nan = np.isnan(logits[row])   # the first NaN, else the first of the maxima (np.argmax returns the first of equal values)
                cls2[i, j] = np.argmax(nan) if nan.any() else np.argmax(logits[row])
                if (cls2[i, j] if class_map is None else class_map[cls2[i, j]]) == labels[i, j]:
                    ob[i, oc[i]], os_[i, oc[i]], ol[i, oc[i]] = boxes[i, j], scores[i, j], labels[i, j]
                    oc[i] += 1
            row += 1
    return ob, os_, ol, oc, cls2, status


def filter_case(name):
    """-> (boxes, scores, labels, counts, logits, total, class_map) as NumPy arrays; every box and score distinct, so a misplaced row shows"""
    g = np.random.default_rng(11)
    k, nc2 = 6, 70                                        # nc2 above a wave's 64 lanes
    counts = {"counts": [0, 1, k, k + 2, -1, 3], "many_images": list(g.integers(0, k + 1, 66)), "total_low": [k, k], "capacity": [k, k]}.get(name, [k, 5, 1])
    n, rows = len(counts), sum(min(max(int(c), 0), k) for c in counts)
    boxes = np.arange(n * k * 4, dtype=np.float32).reshape(n, k, 4)
    scores = (1.0 + np.arange(n * k, dtype=np.float32)).reshape(n, k) / 1024
    labels = g.integers(0, nc2, (n, k)).astype(np.int64)
    cap, class_map = (rows - 3 if name == "capacity" else rows + 2), None
    logits = g.standard_normal((cap, nc2)).astype(np.float32)
    flat = [labels[i, j] for i in range(n) for j in range(min(max(int(counts[i]), 0), k))][:cap]
    for r, lab in enumerate(flat):
        if name == "keep_all" or (name not in ("keep_none", "class_map") and r % 2 == 0):
            logits[r, lab] = 9.0
        elif name == "keep_none":
            logits[r, lab] = -9.0
    if name == "class_map":
        class_map = g.permutation(nc2).astype(np.int32)
        logits[np.arange(0, len(flat), 2), np.argsort(class_map)[flat[::2]]] = 9.0   # (argsort of a permutation is its inverse)
    if name == "ties_nan_inf":
        # rows 0 .. 5: every class ties -> 0; a tie across two strides of a lane -> 5; two NaNs -> the first, whatever else the row holds; all -inf -> 0; -inf but
        # one finite -> it; signed zeros tie -> the first.  Each of them is kept.
        logits[0], logits[1, [5, 69]], logits[2, [66, 3]], logits[3], logits[4], logits[5] = 1.0, 9.5, np.nan, -np.inf, -np.inf, -1.0
        logits[4, 65], logits[5, 7], logits[5, 8] = -3.0e38, 0.0, -0.0
        labels[0, :6] = [0, 5, 3, 0, 65, 7]
    total = np.array([min(rows, cap) - (2 if name == "total_low" else 0), 0], np.int32)
    return boxes, scores, labels, np.array(counts, np.int32), logits, total, class_map


FILTER_CASES = ["counts", "keep_all", "keep_none", "alternating", "class_map", "ties_nan_inf", "many_images", "total_low", "capacity"]
