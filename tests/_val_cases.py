"""The yardstick of tests/test_val_match_gpu.py: a plain NumPy restatement of ymi_val_match's contract (include/yolort_amd.h) and the cases.  Every coordinate is a
multiple of 0.25 below 1024: areas, intersections and unions are exact in fp32 and the division is correctly rounded, so the float32 model is bit-equal to the kernel."""
import numpy as np

F = np.float32
POISON_LABEL = 1 << 40   # in every slot past a count: reading it would raise the bad-label bit


def iou_f32(d, g):
    x1, y1 = np.maximum(d[:, None, 0], g[None, :, 0]), np.maximum(d[:, None, 1], g[None, :, 1])
    x2, y2 = np.minimum(d[:, None, 2], g[None, :, 2]), np.minimum(d[:, None, 3], g[None, :, 3])
    inter = np.maximum(F(0), x2 - x1) * np.maximum(F(0), y2 - y1)
    ad, ag = (d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1]), (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / ((ad[:, None] + ag[None, :]) - inter)
    iou[iou == 0] = 0   # a zero IoU is +0
    return iou


def model(case, conf, thrs, class_aware, all_fp=False):
    """-> match (N,K) int32, iou (N,K) fp32, tp (N,K,T) uint8, matrix (C+1,C+1) int64 (the additions of this batch), status bits"""
    N, K = case["scores"].shape
    C, thr = case["C"], np.asarray(thrs, F)
    match, iou_out = np.full((N, K), -1, np.int32), np.zeros((N, K), F)
    matrix, status = np.zeros((C + 1, C + 1), np.int64), 0
    for i in range(N):
        kd, gn = int(case["counts"][i]), min(max(int(case["gt_counts"][i]), 0), case["gt_labels"].shape[1])
        if kd < 0:
            status |= 2
            continue
        status |= 4 if kd > K else 0
        kd = min(kd, K)
        b, s, l = case["boxes"][i, :kd], case["scores"][i, :kd], case["labels"][i, :kd]
        gb, gl = case["gt_boxes"][i, :gn], case["gt_labels"][i, :gn]
        ok_d, ok_g = (l >= 0) & (l < C), (gl >= 0) & (gl < C)
        status |= 0 if ok_d.all() and ok_g.all() else 1
        iou = iou_f32(b, gb)
        with np.errstate(invalid="ignore"):
            cand = ok_d & (s > F(conf))
            adm = ((iou >= thr[0]) & (l[:, None] == gl[None, :])) if class_aware else (iou > thr[0])
        adm &= cand[:, None] & ok_g[None, :]
        di, gi = np.nonzero(adm)
        v = iou[di, gi]
        o = np.lexsort((gi, -v))                                  # by IoU descending, ties: the lowest ground truth first
        di, gi, v = di[o], gi[o], v[o]
        first = np.unique(di, return_index=True)[1]               # unique by detection: its best ground truth
        di, gi, v = di[first], gi[first], v[first]
        o = np.lexsort((di, -v))                                  # by IoU descending, ties: the lowest slot first
        di, gi, v = di[o], gi[o], v[o]
        first = np.unique(gi, return_index=True)[1]               # unique by ground truth: its best detection
        di, gi, v = di[first], gi[first], v[first]
        match[i, di], iou_out[i, di] = gi, v
        for g in np.nonzero(ok_g)[0]:
            hit = di[gi == g]
            matrix[l[hit[0]] if len(hit) else C, gl[g]] += 1
        if len(di) or all_fp:
            for d in np.nonzero(cand)[0]:
                if d not in di:
                    matrix[l[d], C] += 1
    tp = ((match >= 0)[:, :, None] & (iou_out[:, :, None] >= thr[None, None, :])).astype(np.uint8)
    return match, iou_out, tp, matrix, status


def make_case(images, C, K=None, G=None):
    """images: [(boxes (k,4), scores (k), labels (k), gt_boxes (g,4), gt_labels (g))] -> the padded slab and ground truth, poisoned past the counts"""
    K = max([len(im[1]) for im in images] + [0]) if K is None else K
    G = max([len(im[4]) for im in images] + [0]) if G is None else G
    N = len(images)
    case = dict(C=C, boxes=np.full((N, K, 4), 3e38, F), scores=np.full((N, K), 1e30, F), labels=np.full((N, K), POISON_LABEL, np.int64), counts=np.zeros(N, np.int32),
                gt_boxes=np.full((N, G, 4), 3e38, F), gt_labels=np.full((N, G), -7, np.int32), gt_counts=np.zeros(N, np.int32))
    for i, (b, s, l, gb, gl) in enumerate(images):
        k, g = len(s), len(gl)
        case["boxes"][i, :k], case["scores"][i, :k], case["labels"][i, :k], case["counts"][i] = np.asarray(b, F).reshape(-1, 4), s, l, k
        case["gt_boxes"][i, :g], case["gt_labels"][i, :g], case["gt_counts"][i] = np.asarray(gb, F).reshape(-1, 4), gl, g
    return case


def _boxes(rng, n):
    xy = rng.integers(0, 3200, (n, 2)) / 4.0
    wh = rng.integers(4, 480, (n, 2)) / 4.0
    return np.concatenate([xy, np.minimum(xy + wh, 1023.75)], 1).astype(F)


def random_image(rng, k, g, C):
    """g ground truths, a quarter duplicated (ties in pass 1); k detections, most of them shifted or exact copies of ground truths (ties in pass 2, displaced ones)"""
    gb = _boxes(rng, g)
    if g > 3:
        gb[rng.integers(0, g, g // 4)] = gb[rng.integers(0, g, g // 4)]
    gl = rng.integers(0, C, g).astype(np.int32)
    b = _boxes(rng, k)
    l = rng.integers(0, C, k).astype(np.int64)
    if g and k:
        src = rng.integers(0, g, k)
        near = rng.random(k) < 0.8
        shift = (rng.integers(-12, 13, (k, 4)) * (rng.random((k, 1)) < 0.6) / 4.0).astype(F)
        b[near] = np.clip(gb[src[near]] + shift[near], 0, 1023.75)
        same = near & (rng.random(k) < 0.7)
        l[same] = gl[src[same]]
    return b, (rng.integers(1, 400, k) / 400.0).astype(F), l, gb, gl


def random_case(seed, K, G, C, n_img=3):   # ragged: image 0 is full, the others hold random fractions of K and G (down to nothing)
    rng = np.random.default_rng(seed)
    sizes = [(K, G)] + [(int(rng.integers(0, K + 1)), int(rng.integers(0, G + 1))) for _ in range(n_img - 1)]
    return make_case([random_image(rng, k, g, C) for k, g in sizes], C, K, G)


A, B, Z = [0, 0, 100, 100], [50, 0, 150, 100], [7, 7, 7, 7]
CRAFTED = {   # one scenario per image, C = 3: (boxes, scores, labels, gt_boxes, gt_labels)
    "displaced": ([A, [20, 0, 120, 100]], [0.9, 0.8], [0, 0], [A, B], [0, 0]),   # both prefer A (IoU 1 and 2/3); the loser's second choice B (7/13) is admissible
    "iou on thr0": ([[0, 0, 100, 100]], [0.9], [1], [[0, 0, 100, 50]], [1]),      # IoU exactly 0.5 = thr0: `>` rejects it, `>=` admits it
    "zero area": ([Z, A], [0.9, 0.9], [2, 2], [Z, A], [2, 2]),                     # zero area on zero area: 0 / 0 = NaN matches nothing; on a real box: IoU 0
    "score at conf": ([A, A, A], [0.25, np.nextafter(F(0.25), F(1)), np.nan], [0, 0, 0], [A], [0]),   # at conf (0.25): out; just above: in; NaN: out
    "no match": ([[500, 500, 600, 600], [700, 700, 800, 800]], [0.9, 0.9], [1, 2], [A], [0]),         # candidates, no match: the quirk counts no false positive
    "ties": ([A, A, A], [0.5, 0.7, 0.6], [1, 1, 1], [A, A], [1, 1]),               # both passes: two identical ground truths, three identical detections
    "bad label": ([A, B], [0.9, 0.9], [3, 1], [A, B], [1, -1]),                    # outside [0, C) on either side: skipped, status bit 0
    "confusion": ([A], [0.9], [2], [A], [0]),                                      # the detection sits on a ground truth of another class
}
