"""End-to-end parity of the HIP path against the oracle / reference goldens (MI355X)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _iou(a, b):
    x1, y1 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    x2, y2 = np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter)


def match_fraction(ref, got, iou_thr=0.5, score_tol=0.1, margin=0.0, thr=0.0):
    """(fraction matched, median IoU of matches, max |dscore|): a reference detection is matched
    by a same-label detection with IoU >= iou_thr.  Reference detections whose score is within
    `margin` of the threshold / of the top-k cut are not counted (their survival is decided by
    fp16/bf16 rounding of the conv stack, not by the algorithm)."""
    rb, rs, rl = ref["boxes"], ref["scores"], ref["labels"]
    gb, gs, gl = got["boxes"], got["scores"], got["labels"]
    cut = max(thr, float(rs[-1]) if len(rs) >= 300 else 0.0)
    idx = [i for i in range(len(rs)) if rs[i] >= cut + margin]
    if not idx:
        return 1.0, 1.0, 0.0
    hit, ious_m, ds = 0, [], []
    for i in idx:
        cand = np.where(gl == rl[i])[0]
        if len(cand) == 0:
            continue
        ious = _iou(rb[i], gb[cand])
        j = int(np.nanargmax(ious))
        if ious[j] >= iou_thr and abs(gs[cand[j]] - rs[i]) <= score_tol:
            hit += 1
            ious_m.append(float(ious[j]))
            ds.append(abs(float(gs[cand[j]] - rs[i])))
    return hit / len(idx), float(np.median(ious_m)) if ious_m else 0.0, float(max(ds)) if ds else 0.0


def _np(d):
    return {k: (v.detach().float().cpu().numpy() if k != "labels" else v.detach().cpu().numpy()) for k, v in d.items()}


@pytest.fixture(scope="module")
def dev():
    from yolort_amd import _lib
    _lib.load(require_gpu=True)
    return torch.device("cuda:0")


def _model(arch, dev, dtype, **kw):
    from yolort_amd.models import YOLOv5
    from workloads.synth import synth_weights
    head_gain = kw.pop("head_gain", 0.5)
    m = YOLOv5(arch=arch, **kw)
    m.load_state_dict(synth_weights(m.state_dict(), arch, seed=0, head_gain=head_gain))
    return m.to(dev).to(dtype).eval()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_yolov5n_against_reference_golden(dev, golden_dir, dtype):
    """Same seeded weights/images as tests/golden/e2e_n.npz, which holds the UNMODIFIED reference's
    fp32 CPU outputs.  The conv stack stores fp16/bf16 (fp32 accumulation); its distance to the fp32
    reference is bounded by the distance of the oracle's own fp16/bf16-storage emulation
    (O.EMULATE) to fp32, measured here on the same inputs -- the stated floating-point tolerance."""
    from oracle import yolov5_oracle as O
    from workloads.synth import synth_images, synth_weights
    z = np.load(os.path.join(golden_dir, "e2e_n.npz"))
    S, thr = int(z["S"]), float(z["thr"])
    m = _model("yolov5_darknet_pan_n_r60", dev, dtype, size=(S, S), score_thresh=thr, nms_thresh=0.45, head_gain=float(z["head_gain"]))
    imgs_cpu = [synth_images(1, int(h), int(w), seed=11 + i)[0] for i, (h, w) in enumerate(z["sizes"])]
    dets_fused = m.predict([im.to(dev) for im in imgs_cpu])       # default: decode fused into the head convolution
    m.model.fuse_head_decode = False                               # keep the logits as buffers to compare them below
    dets = m.predict([im.to(dev) for im in imgs_cpu])
    for a, b in zip(dets_fused, dets):                             # both forms must agree bit for bit
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(a[k], b[k]), f"fused / unfused head disagree on {k}"
    e = next(iter(m.model._entries.values()))
    # inherent storage-precision error of this network, from the oracle's emulation mode
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    O.EMULATE.dtype = dtype
    try:
        with torch.no_grad():
            _, emu = O.yolov5_forward([im.to(dtype).float() for im in imgs_cpu], sd, size=(S, S), score_thresh=thr, return_stages=True)
    finally:
        O.EMULATE.dtype = None
    for i, v in enumerate(e.feats):
        got = v.as_tensor().float().cpu().permute(0, 3, 1, 2).numpy()
        ref = z[f"feat{i}"]
        inherent = np.abs(emu["features"][i].numpy() - ref).max()
        err = np.abs(got - ref).max()
        err_emu = np.abs(got - emu["features"][i].numpy()).max()
        print(f"feat{i}: |hip-fp32|={err:.4f} |emu-fp32|={inherent:.4f} |hip-emu|={err_emu:.4f}")
        assert err <= 2.5 * inherent + 1e-3, f"feature {i}: err {err} vs inherent {inherent}"
        assert err_emu <= 2.5 * inherent + 1e-3
    for i, v in enumerate(e.logits):
        n, h, w = v.n, v.h, v.w
        got = v.as_tensor().cpu().view(n, h, w, 3, 85).permute(0, 3, 1, 2, 4).numpy()
        inherent = np.abs(emu["head"][i].numpy() - z[f"head{i}"]).max()
        err = np.abs(got - z[f"head{i}"]).max()
        assert err <= 2.5 * inherent + 1e-3, f"head {i}: abs err {err} vs inherent {inherent}"
    assert len(dets) == 3
    for i, d in enumerate(dets):
        assert list(d.keys()) == ["scores", "labels", "boxes"] and d["labels"].dtype == torch.int64 and d["boxes"].dtype == torch.float32
        ref = {"boxes": z[f"det{i}_boxes"], "scores": z[f"det{i}_scores"], "labels": z[f"det{i}_labels"]}
        loose = dtype == torch.bfloat16
        frac, miou, ds = match_fraction(ref, _np(d), iou_thr=0.5, score_tol=0.15 if loose else 0.05, margin=0.1 if loose else 0.03, thr=thr)
        print(f"image {i}: matched {frac:.3f} median IoU {miou:.4f} max dscore {ds:.4f}")
        assert frac >= (0.6 if loose else 0.93), f"image {i}: only {frac:.3f} of reference detections matched"
        assert miou >= (0.7 if loose else 0.93)


def test_postprocess_exact_given_oracle_logits(dev, golden_dir):
    """Feeding the reference's own fp32 head outputs through the HIP post-process must reproduce
    the reference detections: labels/order bit-exact, boxes within 1e-3 IoU-equivalent tolerance."""
    from oracle import yolov5_oracle as O
    from yolort_amd.ops import postprocess_logits
    z = np.load(os.path.join(golden_dir, "e2e_n.npz"))
    heads = [torch.from_numpy(z[f"head{i}"]).to(dev) for i in range(3)]
    strides, anchors = O.anchors_for(3)
    got = postprocess_logits(heads, strides, anchors, 80, float(z["thr"]), 0.45, 300)
    hb, wb = int(z["batch_shape"][2]), int(z["batch_shape"][3])
    for i, d in enumerate(got):
        boxes = O.scale_coords(d["boxes"].cpu(), (hb, wb), tuple(int(v) for v in z["sizes"][i]))
        np.testing.assert_array_equal(d["labels"].cpu().numpy(), z[f"det{i}_labels"])
        np.testing.assert_allclose(d["scores"].cpu().numpy(), z[f"det{i}_scores"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(boxes.numpy(), z[f"det{i}_boxes"], rtol=1e-5, atol=2e-3)


def test_yolov5s_640_vs_oracle(dev):
    """BASELINE config 2 shape (yolov5s fp16 640x640) at batch 2 against the CPU oracle."""
    from oracle import yolov5_oracle as O
    from workloads.synth import synth_images
    arch = "yolov5_darknet_pan_s_r60"
    m = _model(arch, dev, torch.float16, score_thresh=0.25)
    x = synth_images(2, 640, 640, seed=1)
    dets = m.predict([x[0].to(dev), x[1].to(dev)])
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = O.yolov5_forward([x[0], x[1]], sd, score_thresh=0.25)
    for r, d in zip(ref, dets):
        frac, miou, ds = match_fraction(_np(r), _np(d), margin=0.03, thr=0.25)
        print(f"yolov5s 640: {len(r['scores'])} ref dets, matched {frac:.3f}, median IoU {miou:.4f}, max dscore {ds:.4f}")
        assert len(r["scores"]) > 10
        assert frac >= 0.93 and miou >= 0.93, f"matched {frac:.3f} (max dscore {ds}) of {len(r['scores'])}"


@pytest.mark.parametrize("arch,num_classes,dtype", [("yolov5_darknet_pan_s_r60", 80, torch.float16), ("yolov5_darknet_pan_n_r60", 20, torch.bfloat16),
                                                    ("yolov5_darknet_pan_n_r60", 3, torch.float16), ("yolov5_darknet_pan_n_r60", 100, torch.float16)]
                         + [("yolov5_darknet_pan_n_r60", nc, torch.float16) for nc in (1, 27, 28, 59, 60, 123)])   # 1: one label bit; the others: both sides of every anchor padding (K = 32 / 33, 64 / 65, 128)
def test_fused_head_decode_equals_unfused(dev, arch, num_classes, dtype):
    """ymi_conv_head_decode (decode + threshold in the head conv's epilogue) must produce exactly the records
    the stored-logits path produces: same detections bit for bit, same candidate count; K = num_classes + 5 covers
    every anchor padding (32, 64, 96, 128 rows) and a batch whose 20x20 / 10x10 levels make waves span images"""
    from workloads.synth import synth_images
    m = _model(arch, dev, dtype, num_classes=num_classes, score_thresh=0.2, nms_thresh=0.45)
    x = torch.stack([im for im in synth_images(5, 320, 320, seed=5)]).to(dev).to(dtype)
    outs, ncand = [], []
    for fused in (True, False):
        m.model.fuse_head_decode = fused
        outs.append(m.model(x))
        e = next(iter(m.model._entries.values()))
        assert (e.logits is None) == fused
        ncand.append(int(e.post.status[0].item()))
    assert ncand[0] == ncand[1] and ncand[0] > 0
    for a, b in zip(*outs):
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(a[k], b[k]), f"fused / unfused head disagree on {k}"
    assert sum(len(d["scores"]) for d in outs[0]) > 0


def test_head_of_124_classes_runs_through_stored_logits(dev):
    """num_classes = 124 (K = 129 rows per anchor) is the first count the fused head refuses: the model must store the fp32 head logits and post-process them,
    and its detections must be what ops.postprocess_logits returns for exactly those logits"""
    from workloads.synth import synth_images
    from yolort_amd.ops import postprocess_logits
    nc = 124
    m = _model("yolov5_darknet_pan_n_r60", dev, torch.float16, num_classes=nc, score_thresh=0.2, nms_thresh=0.45)
    x = torch.stack([im for im in synth_images(5, 320, 320, seed=5)]).to(dev).half()
    assert m.model.fuse_head_decode
    out = m.model(x)
    e = next(iter(m.model._entries.values()))
    assert e.logits is not None, "the fused head took 124 classes"
    heads = []
    for v in e.logits:
        t = v.as_tensor()
        heads.append(t.reshape(t.shape[0], t.shape[1], t.shape[2], 3, nc + 5).permute(0, 3, 1, 2, 4).contiguous())
    ag, pp = m.model.anchor_generator, m.model.post_process
    want = postprocess_logits(heads, [float(s) for s in ag.strides], ag.anchor_grids, nc, float(pp.score_thresh), float(pp.nms_thresh), int(pp.detections_per_img))
    assert sum(len(d["scores"]) for d in out) > 0
    for a, b in zip(out, want):
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(a[k], b[k]), f"model / postprocess_logits disagree on {k}"


@pytest.mark.parametrize("k_det", [300, 1500])
def test_score_prefix_selection_is_exact(dev, k_det):
    """Crowded images are post-processed on a score-ordered prefix of their candidates (include/yolort_amd.h,
    YMI_POST_EXACT_FULL): the detections must equal the full computation bit for bit, both when the prefix suffices
    and when it falls short and the host transparently re-runs the batch on the full set (tests/test_ops_gpu.py forces
    that case deterministically)."""
    from workloads.synth import synth_images
    outs, ncand = [], []
    x = torch.stack([im for im in synth_images(2, 640, 640, seed=9)]).to(dev).half()
    for exact in (False, True):
        m = _model("yolov5_darknet_pan_n_r60", dev, torch.float16, score_thresh=0.02, nms_thresh=0.45, detections_per_img=k_det)
        m.model.post_exact_full = exact
        outs.append(m.model(x))
        e = next(iter(m.model._entries.values()))
        ncand.append(int(e.post.status[0].item()))
        if not exact:
            redone = m.model.post_exact_full   # True: the prefix fell short and the host re-ran the batch on the full set
    print("records processed: prefix", ncand[0], "full", ncand[1], "fallback taken:", redone)
    assert ncand[1] > 2 * 6144, "the test needs crowded images"
    if not redone:
        assert ncand[0] < ncand[1], "the prefix selection did not cut anything"
    for a, b in zip(*outs):
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(a[k], b[k]), f"prefix / full post-process disagree on {k}"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_stem_from_planar_equals_letterbox_path(dev, dtype):
    """identity-size batches feed the stem straight from the planar images (ymi_conv_stem_planar): the first feature
    map and the detections must be bit-identical to the letterbox + NHWC4 path; other batches keep the letterbox"""
    from workloads.synth import synth_images
    m = _model("yolov5_darknet_pan_n_r60", dev, dtype, size=(320, 416), score_thresh=0.2, nms_thresh=0.45)
    imgs = [im.to(dev).to(dtype) for im in synth_images(3, 320, 416, seed=21)]
    outs, stems = [], []
    for planar in (True, False):
        m.model.stem_from_planar = planar
        outs.append(m.predict(imgs))
        e = next(iter(m.model._entries.values()))
        e.plan.run(1, 2)   # re-run op 1 only to be sure op 0's output buffer is what the next op consumed
        stems.append(e.plan.conv_descs[0])
    for a, b in zip(*outs):
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(a[k], b[k]), f"planar-stem / letterbox paths disagree on {k}"
    assert sum(len(d["scores"]) for d in outs[0]) > 0
    # a batch that needs real letterboxing must not take the planar path (and must still work)
    m.model.stem_from_planar = True
    odd = [im.to(dev).to(dtype) for im in synth_images(2, 300, 400, seed=22)]
    assert len(m.predict(odd)) == 2


def test_planar_stem_batch_survives_capacity_growth(dev):
    """a planar-stem batch whose candidates overflow the capacity is re-run from the planar images (the NHWC4 input
    buffer is never filled on that path): same detections as the letterbox path with ample capacity"""
    from workloads.synth import synth_images
    imgs = [im.to(dev).half() for im in synth_images(2, 320, 320, seed=31)]
    outs = []
    for planar, cap in ((True, 128), (False, 1 << 16)):
        m = _model("yolov5_darknet_pan_n_r60", dev, torch.float16, size=(320, 320), score_thresh=0.05, nms_thresh=0.45)
        m.model.stem_from_planar = planar
        m.model.cand_cap_per_image = cap
        outs.append(m.predict(imgs))
        if planar:
            assert m.model.cand_cap_per_image > 128, "the capacity should have grown"
    for a, b in zip(*outs):
        assert len(a["scores"]) > 0
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(a[k], b[k]), f"re-run planar batch disagrees on {k}"


def test_predict_accepts_decoded_hwc_uint8(dev):
    """images as a decoder delivers them -- uint8 (H, W, 3) -- give the same detections as their planar (3, H, W) form"""
    from workloads.synth import synth_images
    m = _model("yolov5_darknet_pan_n_r60", dev, torch.float16, size=(320, 320), score_thresh=0.2)
    planar = [(synth_images(1, h, w, seed=91 + i)[0] * 255).round().to(torch.uint8) for i, (h, w) in enumerate([(300, 400), (240, 320)])]
    a = m.predict([u.to(dev) for u in planar])
    b = m.predict([u.permute(1, 2, 0).contiguous().to(dev) for u in planar])
    for x, y in zip(a, b):
        assert len(x["scores"]) > 0
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(x[k], y[k])


def test_mixed_sizes_and_yolo_forward(dev):
    """dynamic-shape letterbox batch + YOLO.forward on a pre-batched tensor (no rescale)."""
    from oracle import yolov5_oracle as O
    from workloads.synth import synth_images
    arch = "yolov5_darknet_pan_n_r60"
    m = _model(arch, dev, torch.float16, size=(320, 320), score_thresh=0.3)
    shapes = [(270, 203), (240, 320), (180, 320), (375, 500)]
    imgs = [synth_images(1, h, w, seed=5 + i)[0] for i, (h, w) in enumerate(shapes)]
    dets = m.predict([im.to(dev) for im in imgs])
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = O.yolov5_forward(imgs, sd, size=(320, 320), score_thresh=0.3)
    for r, d in zip(ref, dets):
        frac, miou, _ = match_fraction(_np(r), _np(d), margin=0.03, thr=0.3)
        assert frac >= 0.9 and miou >= 0.9, (frac, miou)
    xb = synth_images(2, 128, 160, seed=9)
    out = m.model(xb.to(dev).half())
    with torch.no_grad():
        ref2 = O.yolo_forward(xb, sd, 0.3, 0.45, 300, p="model.")
    for r, d in zip(ref2, out):
        frac, miou, _ = match_fraction(_np(r), _np(d), margin=0.03, thr=0.3)
        assert frac >= 0.9 and miou >= 0.9, (frac, miou)


def test_baseline_config1_yolov5n_thr045(dev):
    """BASELINE.json configs[0]: yolov5n score_thresh=0.45 on 2 x 640x640 random images (the reference's own
    CPU-runnable case), here with the seeded synthetic weights so that detections exist."""
    from oracle import yolov5_oracle as O
    from yolort_amd.models import yolov5n
    from workloads.synth import synth_images, synth_weights
    arch = "yolov5_darknet_pan_n_r60"
    m = yolov5n(score_thresh=0.45)
    m.load_state_dict(synth_weights(m.state_dict(), arch, seed=0, head_gain=1.0))
    m = m.to(dev).half().eval()
    imgs = [synth_images(1, 640, 640, seed=i + 1)[0] for i in range(2)]
    dets = m.predict([im.to(dev) for im in imgs])
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = O.yolov5_forward(imgs, sd, score_thresh=0.45)
    for r, d in zip(ref, dets):
        assert len(r["scores"]) > 20
        frac, miou, _ = match_fraction(_np(r), _np(d), margin=0.03, thr=0.45)
        assert frac >= 0.9 and miou >= 0.93, (frac, miou, len(r["scores"]))


def test_baseline_config3_yolov5m_bf16_dynamic_1280(dev):
    """BASELINE.json configs[2] at reduced batch: yolov5m bf16, size (1280,1280), images whose shapes hit the
    letterbox rounding traps -> per-image bilinear gather + common canvas."""
    from oracle import yolov5_oracle as O
    from yolort_amd.models import yolov5m
    from workloads.synth import synth_images, synth_weights
    arch = "yolov5_darknet_pan_m_r60"
    m = yolov5m(size=(1280, 1280), score_thresh=0.3)
    m.load_state_dict(synth_weights(m.state_dict(), arch, seed=0, head_gain=2.0))   # m / l6 are calibrated at 1280 (oracle/make_synth_bn.py): sane activations need a larger head gain
    m = m.to(dev).to(torch.bfloat16).eval()
    shapes = [(641, 480), (375, 500), (1281, 1279)]
    imgs = [synth_images(1, h, w, seed=31 + i)[0] for i, (h, w) in enumerate(shapes)]
    dets = m.predict([im.to(dev) for im in imgs])
    e = next(iter(m.model._entries.values()))
    assert (e.x.h, e.x.w) == (1280, 1280)   # canvas of the mixed batch
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = O.yolov5_forward(imgs, sd, size=(1280, 1280), score_thresh=0.3)
    assert sum(len(r["scores"]) for r in ref) > 30
    for r, d in zip(ref, dets):
        frac, miou, _ = match_fraction(_np(r), _np(d), iou_thr=0.5, score_tol=0.15, margin=0.1, thr=0.3)
        assert frac >= 0.6 and miou >= 0.7, (frac, miou, len(r["scores"]))


def test_uint8_ingest_matches_float_path(dev):
    """uint8 images: /255 is fused into the letterbox kernel; same detections as feeding x/255."""
    from workloads.synth import synth_images
    m = _model("yolov5_darknet_pan_n_r60", dev, torch.float16, size=(320, 320), score_thresh=0.3, head_gain=1.0)
    u8 = [(synth_images(1, 240, 320, seed=7)[0] * 255).round().to(torch.uint8), (synth_images(1, 300, 200, seed=8)[0] * 255).round().to(torch.uint8)]
    a = m.predict([u.to(dev) for u in u8])
    b = m.predict([(u.float() / 255.0).to(dev) for u in u8])
    # the float path rounds x/255 to fp16 before the resize, the uint8 path after it: same detections up to that rounding
    for x, y in zip(a, b):
        frac, miou, ds = match_fraction(_np(y), _np(x), margin=0.02, thr=0.3, score_tol=0.02)
        assert frac >= 0.97 and miou >= 0.97, (frac, miou, ds)


def test_async_pipeline_matches_sync(dev):
    """several batches in flight (forward_async) return exactly what the synchronous calls return"""
    from workloads.synth import synth_images
    m = _model("yolov5_darknet_pan_n_r60", dev, torch.float16, size=(160, 160), score_thresh=0.3, head_gain=1.0)
    batches = [[synth_images(1, 128, 160, seed=50 + 2 * i)[0].to(dev), synth_images(1, 160, 120, seed=51 + 2 * i)[0].to(dev)] for i in range(6)]
    sync = [m.forward(b) for b in batches]
    pend = [m.forward_async(b) for b in batches[:3]]
    out = [p.result() for p in pend]
    pend = [m.forward_async(b) for b in batches[3:]]
    out += [p.result() for p in pend]
    for s_, o_ in zip(sync, out):
        for x, y in zip(s_, o_):
            assert torch.equal(x["labels"], y["labels"]) and torch.equal(x["scores"], y["scores"]) and torch.equal(x["boxes"], y["boxes"])


def test_p6_model_runs(dev):
    from oracle import yolov5_oracle as O
    from workloads.synth import synth_images
    arch = "yolov5_darknet_pan_l6_r60"
    m = _model(arch, dev, torch.float16, size=(256, 256), size_divisible=64, score_thresh=0.3, head_gain=3.0)
    imgs = [synth_images(1, 200, 256, seed=3)[0]]
    dets = m.predict([imgs[0].to(dev)])
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = O.yolov5_forward(imgs, sd, size=(256, 256), size_divisible=64, score_thresh=0.3)
    assert len(ref[0]["scores"]) > 10
    frac, miou, _ = match_fraction(_np(ref[0]), _np(dets[0]), margin=0.03, thr=0.3)
    assert frac >= 0.9 and miou >= 0.9, (frac, miou)


def test_api_errors(dev):
    from yolort_amd._lib import YmiError
    from yolort_amd.models import yolov5n
    m = yolov5n().to(dev).half().eval()
    with pytest.raises(ValueError):
        m.predict(torch.rand(2, 3, 64, 64, device=dev))  # 4-D tensor to predict (reference Appendix G)
    with pytest.raises(NotImplementedError):
        m.predict({"a": 1})
    with pytest.raises(YmiError):
        m.forward([torch.rand(3, 64, 64)])  # CPU tensor: no fallback
    out = m.predict(torch.rand(3, 64, 64, device=dev))
    assert out[0]["boxes"].shape == (0, 4) and out[0]["scores"].shape == (0,) and out[0]["labels"].dtype == torch.int64


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_sharded_dynamic_shape_batch_on_the_global_canvas_equals_the_whole_batch(dev, dtype):
    """SURVEY.md 8e / reference transform.py:307-314: the reference pads to the maximum over the WHOLE list.  A list of differently shaped images is run (a) as one
    batch and (b) as two shards whose own canvases differ from each other, each letterboxed onto the canvas of the whole list (`canvas=`, what every rank of a
    sharded stream passes: transform.canvas_of / dist.agree_canvas): the shards' detections equal the whole batch's BIT FOR BIT (an image's computation does not
    depend on its batch neighbours once the canvas is fixed); on their own canvases they differ.  fp32 mode: shards of two images against the batch of four (every
    fp32 tile sums in the same order, so the batch size does not matter either); fp16: the shards are filled up to the whole batch's size with copies, so that both
    runs take the same plan (16-bit plans of different batch sizes may pick tiles that accumulate K in another order)."""
    from workloads.synth import synth_images
    arch, S = "yolov5_darknet_pan_s_r60", 320
    m = _model(arch, dev, torch.float16 if dtype == torch.float16 else torch.float32, size=(S, S), score_thresh=0.2, head_gain=0.5)
    if dtype == torch.float32:
        m = m.float().set_compute_dtype(torch.float32)
    shapes = [(200, 320), (150, 320), (320, 180), (120, 240)]      # shard 0: two landscape images (canvas 224 x 320), shard 1: a portrait and a small one (320 x 192 -> 320 x 320)
    imgs = [synth_images(1, h, w, seed=60 + i)[0].to(dev).to(dtype) for i, (h, w) in enumerate(shapes)]
    t = m.transform
    whole_canvas = t.canvas_of(shapes)
    local = [t.canvas_of(shapes[:2]), t.canvas_of(shapes[2:])]
    assert local[0] != whole_canvas and local[0] != local[1]
    fill = 1 if dtype == torch.float32 else 2
    sh0, sh1 = imgs[:2] * fill, imgs[2:] * fill
    whole = [_np(d) for d in m.forward(imgs)]
    shards = [_np(d) for d in m.forward(sh0, canvas=whole_canvas)[:2]] + [_np(d) for d in m.forward(sh1, canvas=whole_canvas)[:2]]
    assert sum(len(d["scores"]) for d in whole) >= 8
    for a, b in zip(whole, shards):
        assert np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["scores"], b["scores"]) and np.array_equal(a["boxes"], b["boxes"])
    own = [_np(d) for d in m.forward(sh0)[:2]] + [_np(d) for d in m.forward(sh1)[:2]]
    assert any(a["scores"].shape != b["scores"].shape or not np.array_equal(a["boxes"], b["boxes"]) for a, b in zip(whole[:2], own[:2]))   # shard 0's own canvas is 224 x 320
    with pytest.raises(ValueError):
        m.forward(imgs, canvas=(64, 64))
