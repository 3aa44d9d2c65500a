"""Shared by tests/test_head_exact_gpu.py (the real kernels) and tests/test_hipsim_kernels.py (the same sources on the CPU simulator): inputs of the FUSED detection head
(yolort_amd/csrc/head_decode.hpp: the 1x1 head convolution with sigmoid, anchor decode, multi-label threshold and candidate compaction in its epilogue) whose logits are
known EXACTLY, and the conditions, computed from the oracle's decode alone, under which a case says anything.

Why the logits are exact.  Every pixel's input vector holds exactly one 1.0 per 32-channel block and zeros elsewhere, the weights are values exact in fp16 AND bf16
(integers, quarters below 8, multiples of 2^-6 below 2), the bias is fp32.  A logit is then W[c, j1] + W[c, j2] + ... + bias[c]: at most nine terms, each a multiple of
2^-10, the sum of their magnitudes below 2^13 -- every partial sum in every order is exact in fp32.  The fp32 accumulation of the kernel has nothing to round, numpy
states the logits bit for bit, and the expected detections are O.postprocess(O.decode(logits)) with no convolution error to budget.

A block-0 column is a pixel KIND: the kinds of a level are its palette (sparse kinds with a few passing classes, dense kinds that pass every (anchor, class) pair, a hot
kind for the last pixel, an empty kind), the columns of the other blocks add small exact offsets so that a K loop that drops or repeats a block changes the logits."""
import functools

import numpy as np
import torch

# per-wave LDS capacities of the fused head: HdCfg<NA> in yolort_amd/csrc/head_decode.hpp (NA = anchors per wave: 1 = the anchor-split default, 3 = YOLORT_AMD_HEAD_SPLIT=0)
HD_BUF_NA1, HD_WL_NA1 = 256, 256      # records per wave buffer / worklist entries per wave
HD_BUF_NA3, HD_WL_NA3 = 1024, 512
WAVE_PIXELS = 32                      # a wave owns 32 consecutive pixels of the level's n * h * w
NEAR_REL = 4e-6                       # twice the score tolerance of the post-process tests (rtol 2e-6): one ulp of expf cannot flip a count

F32 = np.float32
HALF, QUARTER = float(F32(0.5)), float(F32(0.25))
BELOW_HALF, BELOW_QUARTER = float(np.nextafter(F32(0.5), F32(0))), float(np.nextafter(F32(0.25), F32(0)))

G3 = dict(n=3, shapes=[(8, 16), (5, 7), (1, 3)], chans=[32, 96, 256])   # n*h*w = 384 (whole 128-pixel blocks), 105 (35 pixels an image: waves span two images), 9 (one partial wave)
DENSE3 = [(0, 0), (1, 32), (0, 352)]   # (level, first pixel) of the all-pass 32-pixel runs: the start of a level, across the image 0 / 1 boundary (35), ending at pixel M - 1
COVER = ("last-pixel", "coverage")

CLASS_COUNTS_F16 = (1, 27, 28, 59, 60, 91, 92, 123)   # both sides of each anchor padding (TNA = 1 ... 4: K = nc + 5 = 32 | 33, 64 | 65, 96 | 97, 128) and the one-label-bit count
CLASS_COUNTS_BF16 = (27, 28, 123)


def _specs():
    s = {}
    for dt, counts in (("float16", CLASS_COUNTS_F16), ("bfloat16", CLASS_COUNTS_BF16)):
        for nc in counts:
            s[f"nc{nc}-{dt}"] = dict(G3, nc=nc, dtype=dt, dense=[(1, 32)], guards=COVER + ("two-images",) + (("buf-na1", "buf-na3") if nc >= 27 else ()))
    s["dense"] = dict(G3, nc=27, dense=DENSE3, wide=True, guards=COVER + ("two-images", "buf-na1", "buf-na3", "dense-positions"))
    s["levels-1"] = dict(n=4, shapes=[(5, 7)], chans=[96], nc=11, dense=[(0, 32)], guards=COVER + ("two-images", "buf-na1"))
    s["levels-2"] = dict(n=2, shapes=[(8, 16), (5, 7)], chans=[256, 32], nc=11, dense=[(1, 32)], wide=True, guards=COVER + ("two-images", "buf-na1"))
    s["levels-4"] = dict(n=3, shapes=[(8, 16), (5, 7), (2, 3), (1, 3)], chans=[32, 96, 256, 32], nc=11, dense=[(1, 32)], guards=COVER + ("two-images", "buf-na1"))
    # the palette: logit 0 -> sigmoid 0.5, +20 -> 1.0, -20 -> "fails"; objectness logit 0, classes (20, 0, -20): the scores are exactly 0.5 and 0.25 in any implementation
    tie = dict(n=2, shapes=[(5, 7)], chans=[32], nc=3, design="palette", exact=(0.25, 0.5), guards=())
    s["tie-half"] = dict(tie, thr=HALF, expect_candidates=0, guards=("tie",))
    s["tie-below-half"] = dict(tie, thr=BELOW_HALF, expect_candidates=210, guards=("two-images",))   # also objectness one ulp above thr: p = 1 - 2^-24, class logit 20 must survive the pre-filter
    s["tie-quarter"] = dict(tie, thr=QUARTER, expect_candidates=210, guards=("tie", "two-images"))
    s["tie-below-quarter"] = dict(tie, thr=BELOW_QUARTER, expect_candidates=420, guards=("two-images",))
    s["palette-mixed"] = dict(G3, nc=3, design="palette-mixed", exact=(0.25, 0.5, 1.0), thr=HALF, guards=("tie", "two-images", "last-pixel"))   # objectness 0 or 20: scores 1.0 pass, 0.5 tie, 0.25 fail
    small = dict(n=3, shapes=[(5, 7), (1, 3)], chans=[32, 96], nc=3, design="domain")
    s["thr-zero"] = dict(small, thr=0.0, exact=(0.0,), guards=("tie", "two-images", "last-pixel", "zero-scores"))       # a score of exactly 0 (class logits <= -104) must not pass
    s["thr-negative"] = dict(small, thr=-1.0, guards=("two-images", "last-pixel", "zero-scores", "everything"))   # every (anchor, class) pair of every pixel passes
    s["global-sink"] = dict(G3, nc=3, thr=0.7, cand_cap=180, guards=COVER + ("global-sink",))              # cand_cap / n < 64: one global candidate list
    s["overflow"] = dict(G3, nc=27, dense=DENSE3, cand_cap=3 * 1024, guards=("buf-na1", "overflow"))       # per-image regions of 1024 records, thousands of candidates
    s["nms"] = dict(G3, nc=27, dense=DENSE3, nms=0.45, k=50, guards=COVER + ("truncates",))
    return s


SPECS = _specs()
SEEDS = {}   # name -> seed where the default (0) leaves a score within NEAR_REL of the threshold; found on the CPU (assert_head_case_is_not_vacuous checks it)

GPU_CASES = tuple(SPECS)
NA3_CASES = ("dense", "tie-below-quarter", "nc27-float16", "nc59-float16", "nc91-float16", "nc123-float16")   # the child process: dense, a tie, one class count per TNA
SIM_SPECS = {   # the CPU simulator (a run costs ~15 s whatever its size): the smallest geometry that keeps the guards true -- one 5 x 7 level, two images, 9 classes (32 * 9 > 256)
    "sim-dense": dict(n=2, shapes=[(5, 7)], chans=[96], nc=9, dense=[(0, 32)], guards=COVER + ("two-images", "buf-na1")),
    "sim-tie-below-quarter": dict(SPECS["tie-below-quarter"]),
    "sim-thr-negative": dict(n=2, shapes=[(5, 7), (1, 3)], chans=[32, 64], nc=3, design="domain", thr=-1.0, guards=("two-images", "last-pixel", "zero-scores", "everything")),
}


def _grid(rng, shape, step, lim):
    """multiples of `step` in [-lim, lim]"""
    m = int(round(lim / step))
    return (rng.integers(-m, m + 1, shape) * step).astype(F32)


def _kinds(rng, design, nc):
    """block-0 columns (3, K, 32): logits of the 32 pixel kinds of a level (before the other blocks' offsets and the bias) -> (columns, sparse kinds, dense kinds, hot kind)"""
    k0 = np.zeros((3, nc + 5, 32), F32)
    k0[:, :4] = _grid(rng, (3, 4, 32), 2.0 ** -6, 1.5)
    if design == "random":
        k0[:, 4] = rng.integers(-4, 2, (3, 32))
        cls = np.full((3, nc, 32), -6.0, F32)
        hit = rng.random((3, nc, 32)) < min(1.0, 2.5 / nc)
        cls[hit] = rng.integers(0, 5, int(hit.sum()))
        k0[:, 5:] = cls
        for kd in (28, 29):   # dense: every (anchor, class) passes; rounded class logits: exact score ties inside the run
            k0[:, 4, kd] = 6.0
            k0[:, 5:, kd] = np.clip(5.0 + np.round(rng.standard_normal((3, nc))) * 0.25, 4.0, 6.0)
        k0[:, 4, 30] = 5.0     # hot: every pair passes, every class with its own score step
        k0[:, 5:, 30] = 4.0 + rng.integers(0, 5, (3, nc)) * 0.5
        k0[:, 4, 31] = -20.0   # empty
        return k0, np.arange(28), np.array([28, 29]), 30
    if design == "palette":
        k0[:, 4] = 0.0
        k0[:, 5:] = np.array([20.0, 0.0, -20.0], F32)[None, :, None]
    elif design == "palette-mixed":
        k0[:, 4] = rng.choice(np.array([0.0, 20.0], F32), (3, 32))
        k0[:, 5:] = rng.choice(np.array([20.0, 0.0, -20.0], F32), (3, nc, 32))
        k0[:, 4, 30], k0[:, 5:, 30] = 20.0, 20.0
    elif design == "domain":   # sigmoid(<= -104) is 0 in fp32 (exp overflows); nothing lies between -20 and -104 (subnormal sigmoids)
        k0[:, 4] = rng.choice(np.array([0.0, 20.0, -104.0, 2.0, -3.0], F32), (3, 32))
        k0[:, 5:] = rng.choice(np.array([20.0, 0.0, -20.0, -104.0, -110.0, 3.0, -2.0], F32), (3, nc, 32))
        k0[:, 4, 30] = 2.0
        k0[:, 5:, 30] = np.array([3.0, -104.0, -2.0], F32)[None, :]
    else:
        raise KeyError(design)
    return k0, np.arange(32), np.array([30]), 30


@functools.lru_cache(maxsize=None)
def head_case(name):
    """-> dict: x [(n, h, w, cin) f32 of 0 / 1] per level, weight [(3K, cin)] / bias [(3K,)] per level in nn.Conv2d order (row = anchor * K + output), logits
    [(n, 3, h, w, K)] in the reference layout (exact), pred / candidates from the oracle's decode, and n, nc, shapes, chans, strides, anchors, thr, nms, k, cand_cap, dtype,
    wide (the input is to be given as a channel slice of a wider buffer), tie, guards.  Cached: the tests share one reference and leave it unchanged."""
    from oracle import yolov5_oracle as O
    spec = dict(SPECS.get(name) or SIM_SPECS[name])
    rng = np.random.default_rng([SEEDS.get(name, 0), sum(ord(ch) * (i + 1) for i, ch in enumerate(name))])
    n, nc, shapes, chans = spec["n"], spec["nc"], spec["shapes"], spec["chans"]
    design, kk = spec.get("design", "random"), nc + 5
    strides, anchors = O.anchors_for(4 if len(shapes) == 4 else 3)
    strides, anchors = list(strides[: len(shapes)]), [list(map(float, a)) for a in anchors[: len(shapes)]]
    xs, ws, bs, logits = [], [], [], []
    for lvl, ((h, w), cin) in enumerate(zip(shapes, chans)):
        m_all, blocks = n * h * w, cin // 32
        k0, sparse, dense, hot = _kinds(rng, design, nc)
        wt = np.zeros((3, kk, cin), F32)
        wt[:, :, :32] = k0
        for b in range(1, blocks):   # the other blocks: small offsets (boxes on the 2^-6 grid, objectness / classes on the 2^-3 grid: few distinct scores)
            wt[:, :4, 32 * b: 32 * b + 32] = _grid(rng, (3, 4, 32), 2.0 ** -6, 0.5)
            if not design.startswith("palette"):   # the palette's objectness / class logits stay 0 and +-20
                wt[:, 4:, 32 * b: 32 * b + 32] = _grid(rng, (3, kk - 4, 32), 2.0 ** -3, 0.25)
        bias = np.zeros((3, kk), F32)
        bias[:, :4] = _grid(rng, (3, 4), 2.0 ** -10, 0.25)   # not representable in 16 bits: the bias is added in fp32
        if design == "random":
            bias[:, 4:] = _grid(rng, (3, kk - 4), 2.0 ** -3, 0.25)
        kind = rng.choice(sparse, m_all)
        if design == "random":
            kind[rng.random(m_all) < 0.1] = 31
        for dl, start in spec.get("dense", ()):
            if dl == lvl:
                kind[start: start + WAVE_PIXELS] = rng.choice(dense, WAVE_PIXELS)
        if design != "palette" and not any(dl == lvl and start + WAVE_PIXELS >= m_all for dl, start in spec.get("dense", ())):
            kind[m_all - 1] = hot
        x = np.zeros((m_all, cin), F32)
        x[np.arange(m_all), kind] = 1.0
        for b in range(1, blocks):
            x[np.arange(m_all), 32 * b + rng.integers(0, 32, m_all)] = 1.0
        w2 = wt.reshape(3 * kk, cin)
        # exactness: operands exact in both 16-bit types, every term a multiple of 2^-10, magnitudes summing below 2^13 (so every partial sum in any order is exact in fp32)
        tw = torch.from_numpy(w2)
        assert torch.equal(tw.half().float(), tw) and torch.equal(tw.bfloat16().float(), tw), f"{name}: a weight is not exact in fp16 and bf16"
        terms = np.concatenate([w2.reshape(-1), bias.reshape(-1)]).astype(np.float64) * 1024.0
        assert (terms == np.round(terms)).all() and blocks * np.abs(w2).max() + np.abs(bias).max() < 2.0 ** 13
        lg64 = x.astype(np.float64) @ w2.astype(np.float64).T + bias.reshape(-1).astype(np.float64)
        lg = lg64.astype(F32)
        assert (lg.astype(np.float64) == lg64).all()
        xs.append(x.reshape(n, h, w, cin))
        ws.append(w2)
        bs.append(bias.reshape(-1))
        logits.append(torch.from_numpy(lg.reshape(n, h, w, 3, kk)).permute(0, 3, 1, 2, 4).contiguous())
    thr = float(spec.get("thr", 0.3))
    pred = O.decode(logits, strides, anchors)
    cand = (pred[..., 5:] * pred[..., 4:5]) > thr          # (n, anchors, nc): box_head.py:357, :418
    per_image = cand.sum((1, 2))
    k = int(spec.get("k") or (int(per_image.max()) + 64) // 64 * 64 + 64)
    return dict(name=name, dtype=getattr(torch, spec.get("dtype", "float16")), n=n, nc=nc, shapes=shapes, chans=chans, strides=strides, anchors=anchors, thr=thr,
                nms=float(spec.get("nms", 1.0)), k=k, cand_cap=int(spec.get("cand_cap", n * 16384)), wide=bool(spec.get("wide", False)), tie="tie" in spec["guards"],
                guards=spec["guards"], exact=tuple(spec.get("exact", ())), expect_candidates=spec.get("expect_candidates"), dense=list(spec.get("dense", ())), design=design,
                x=xs, weight=ws, bias=bs, logits=logits, pred=pred, cand=cand, candidates_per_image=per_image.tolist())


@functools.lru_cache(maxsize=None)
def head_reference(name):
    """the oracle's detections of a case: O.postprocess(O.decode(logits, strides, anchors), thr, nms, k), from the exact logits alone"""
    from oracle import yolov5_oracle as O
    c = head_case(name)
    return O.postprocess(c["pred"], c["thr"], c["nms"], c["k"])


def make_head(case):
    """a YOLOHead holding the case's weights and bias (pack with .packed_anchor_major for the fused head, .packed for the unfused convolution)"""
    from yolort_amd.models.box_head import YOLOHead
    head = YOLOHead(list(case["chans"]), 3, [int(s) for s in case["strides"]], case["nc"]).eval()
    with torch.no_grad():
        for m, w, b in zip(head.head, case["weight"], case["bias"]):
            m.weight.copy_(torch.from_numpy(w).view(m.weight.shape))
            m.bias.copy_(torch.from_numpy(b))
    return head


def records_per_wave(case):
    """per level (3, waves): candidates of each (anchor, wave-aligned 32-pixel run), and per level (waves,) the number of images with candidates among the run's pixels"""
    cand, n = case["cand"], case["n"]
    per_level, images, off = [], [], 0
    for h, w in case["shapes"]:
        hw, m_all = h * w, n * h * w
        cnt = cand[:, off: off + 3 * hw].sum(-1).view(n, 3, hw).permute(1, 0, 2).reshape(3, m_all)   # (anchor, pixel m = img * hw + y * w + x)
        waves = (m_all + WAVE_PIXELS - 1) // WAVE_PIXELS
        pad = torch.zeros(3, waves * WAVE_PIXELS, dtype=cnt.dtype)
        pad[:, :m_all] = cnt
        per_level.append(pad.view(3, waves, WAVE_PIXELS).sum(-1))
        has = pad.sum(0) > 0
        img = torch.arange(waves * WAVE_PIXELS) // hw
        images.append(torch.tensor([len(set(img[wv * WAVE_PIXELS: (wv + 1) * WAVE_PIXELS][has[wv * WAVE_PIXELS: (wv + 1) * WAVE_PIXELS]].tolist())) for wv in range(waves)]))
        off += 3 * hw
    return per_level, images


def assert_head_case_is_not_vacuous(case, ref=None):
    """from the ORACLE's decode alone (and, for the truncating case, its detections): the case reaches what it is there to reach, and -- for EVERY case, no exceptions --
    no score other than a designed tie lies within a relative NEAR_REL of the threshold.  -> a line of figures to print"""
    name, thr, n, nc, guards = case["name"], F32(case["thr"]), case["n"], case["nc"], case["guards"]
    scores = (case["pred"][..., 5:] * case["pred"][..., 4:5]).numpy()
    ties = scores == thr
    designed = np.isin(scores, np.array(case["exact"], F32))   # palette scores: 0.25, 0.5 and 1.0 (0 in the threshold-domain case) are exact in any implementation
    near = (np.abs(scores.astype(np.float64) - float(thr)) <= NEAR_REL * abs(float(thr))) & ~designed
    assert not near.any(), f"{name}: {int(near.sum())} scores within {NEAR_REL} (relative) of the threshold {thr!r}: {scores[near][:5]}"
    assert ties.any() == case["tie"] and (designed | ~ties).all(), f"{name}: {int(ties.sum())} scores equal the threshold"
    cand = case["cand"]
    assert int(cand.sum()) > 0 or case["expect_candidates"] == 0, f"{name}: no candidate at all"
    if case["expect_candidates"] is not None:
        assert int(cand.sum()) == case["expect_candidates"], (name, int(cand.sum()))
    per_level, images = records_per_wave(case)
    densest_na1 = max(int(p.max()) for p in per_level)
    densest_na3 = max(int(p.sum(0).max()) for p in per_level)
    if "buf-na1" in guards:   # the pre-filter is a superset of the records: more records than WL <= BUF also spills the worklist
        assert densest_na1 > max(HD_BUF_NA1, HD_WL_NA1), f"{name}: the densest (run, anchor) has {densest_na1} records"
    if "buf-na3" in guards:
        assert densest_na3 > max(HD_BUF_NA3, HD_WL_NA3), f"{name}: the densest run has {densest_na3} records over the three anchors"
    if "dense-positions" in guards:
        for lvl, start in case["dense"]:
            assert int(per_level[lvl][:, start // WAVE_PIXELS].min()) > HD_BUF_NA1, (name, lvl, start)
        m0 = n * case["shapes"][0][0] * case["shapes"][0][1]
        assert (0, 0) in case["dense"] and (0, m0 - WAVE_PIXELS) in case["dense"] and m0 % 128 == 0
        assert any(int(images[lvl][start // WAVE_PIXELS]) >= 2 for lvl, start in case["dense"])
    if "two-images" in guards:
        assert max(int(i.max()) for i in images) >= 2, f"{name}: no wave holds candidates of two images"
    off = 0
    last_pixel, level_hit, anchor_hit = False, [], [False] * 3
    for h, w in case["shapes"]:
        lv = cand[:, off: off + 3 * h * w].view(n, 3, h * w, nc)
        last_pixel |= bool(lv[n - 1, :, h * w - 1].any())
        level_hit.append(bool(lv.any()))
        anchor_hit = [a or bool(lv[:, q].any()) for q, a in enumerate(anchor_hit)]
        off += 3 * h * w
    if "last-pixel" in guards:
        assert last_pixel, f"{name}: pixel M - 1 of no level has a candidate"
    if "coverage" in guards:
        assert all(level_hit) and all(anchor_hit) and bool(cand[..., 0].any()) and bool(cand[..., nc - 1].any()), (name, level_hit, anchor_hit)
    if "zero-scores" in guards:   # a score of exactly 0 under a positive objectness: the anchor is not skipped as a whole, the class itself has to be refused
        assert ((scores == 0) & (case["pred"][..., 4:5].numpy() > 0)).any(), f"{name}: no zero score under a positive objectness"
    if "everything" in guards:
        assert bool(cand.all())
    if "global-sink" in guards:
        assert case["cand_cap"] // n < 64 and 0 < int(cand.sum()) <= case["cand_cap"], (name, int(cand.sum()))
    if "overflow" in guards:
        assert int(cand.sum()) > case["cand_cap"] and case["cand_cap"] // n >= 64
    if "truncates" in guards:
        assert ref is not None and all(len(r["scores"]) == case["k"] for r in ref) and case["nms"] < 1.0
        assert all(int(c) > 4 * case["k"] for c in case["candidates_per_image"])
        from oracle import yolov5_oracle as O
        plain = O.postprocess(case["pred"], case["thr"], 1.0, case["k"])   # the top k without suppression
        assert all(not torch.equal(r["scores"], p_["scores"]) for r, p_ in zip(ref, plain)), f"{name}: the NMS suppresses nothing among the top {case['k']}"
    return (f"{name}: candidates {case['candidates_per_image']} k={case['k']} densest (run, anchor) {densest_na1} / run {densest_na3} "
            f"images per wave <= {max(int(i.max()) for i in images)} ties {int(ties.sum())}")


# ---- the real kernels through the C ABI (tests/test_head_exact_gpu.py and the YOLORT_AMD_HEAD_SPLIT=0 child process it starts) ---------------------------------------------
HEAD_MODES = ("group", "single", "unfused")
WIDE_PAD, WIDE_VALUE = 32, 1000.0   # channels on either side of a `wide` input and what they hold: a read outside the view's cin channels changes the logits by thousands


def _gpu_head_pass(dev, case, head, mode, cap, flags, fill):
    """one pass of one form on a fresh plan -> PostBuffers.  group: post_begin, ymi_conv_head_decode_group, post_finish; single: ymi_conv_head_decode once per level;
    unfused: ymi_postprocess on the exact logits uploaded as fp32 (decode_kernel)"""
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
        pb = plan.postprocess(views, *args, flags=flags)
    else:
        xs, pcs = [], []
        for i, x in enumerate(case["x"]):
            _, h, w, cin = x.shape
            if case["wide"]:   # a channel slice of a wider plan buffer whose other channels hold large finite values
                buf = plan.alloc(n, h, w, cin + 2 * WIDE_PAD)
                buf.as_tensor().fill_(WIDE_VALUE)
                v = buf.slice_c(WIDE_PAD, cin)
            else:
                v = plan.alloc(n, h, w, cin)
            v.as_tensor().copy_(torch.from_numpy(x).to(dev))
            xs.append(v)
            pcs.append(head.packed_anchor_major(i, dtype, dev, cin))
        pb, d = plan.post_desc(case["shapes"], n, *args, flags=flags)
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
    pb.plan = plan   # the buffers live as long as their plan
    return pb


def gpu_head(dev, case, mode, fill=-3.0):
    """one form of the head + post-process under the host protocol of yolort_amd/ops.py::postprocess_logits (tests/test_ops_gpu.py::_gpu_post): a too small candidate capacity
    is grown, a short score prefix is followed by the exact full pass, and the batch redone -> dict(count, labels, scores, boxes: CPU tensors of the last pass, slots past the
    counts still `fill`; passes: the status words of every pass; cap: the final capacity)"""
    from yolort_amd import _lib
    head = None if mode == "unfused" else make_head(case)
    n, cap, flags, passes = case["n"], case["cand_cap"], 0, []
    while True:
        pb = _gpu_head_pass(dev, case, head, mode, cap, flags, fill)
        st = pb.status.cpu().tolist()
        passes.append(st)
        assert len(passes) <= 6, passes
        if st[1] == 0:
            return dict(count=pb.count.cpu(), labels=pb.labels.cpu(), scores=pb.scores.cpu(), boxes=pb.boxes.cpu(), passes=passes, cap=cap)
        if not st[1] & 1:
            flags = _lib.POST_EXACT_FULL
            continue
        need = max(st[0], st[3] * n)
        cap = max(int(need * 1.25) + 1024, 2 * cap)
        cap = n * (1 << ((cap + n - 1) // n - 1).bit_length())


def assert_equals_oracle(got, ref, fill):
    """counts, labels, order exact; scores / boxes to the rounding of expf (the constants of tests/test_ops_gpu.py::_assert_post_equals_oracle); slots past the counts untouched"""
    for i, r in enumerate(ref):
        c = int(got["count"][i])
        assert c == len(r["scores"]), (i, c, len(r["scores"]))
        np.testing.assert_array_equal(got["labels"][i, :c].numpy(), r["labels"].numpy())
        np.testing.assert_allclose(got["scores"][i, :c].numpy(), r["scores"].numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(got["boxes"][i, :c].numpy(), r["boxes"].numpy(), rtol=1e-5, atol=1e-4)
        assert (got["scores"][i, c:] == fill).all() and (got["labels"][i, c:] == int(fill)).all() and (got["boxes"][i, c:] == fill).all(), f"image {i}: slots past the count were written"
