"""Throughput benchmark of the MI355X YOLOv5 inference hot path (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W                      (BASELINE configs[1]: yolov5s fp16 bs 32 640x640)
    python bench.py --config c3|c5|c1 ...                              (the other BASELINE configs, see CONFIGS below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A "step" is one pass of the whole hot path over one batch of synthetic images per GPU: letterbox -> CSPDarknet+PAN ->
head -> decode + class-aware NMS + top-k + rescale -> List[Dict], with the images already resident in HBM.  With N > 1
every rank runs its own shard (weak scaling: `batch` images per GPU) and the fixed-shape detection slabs are all-gathered
over RCCL.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times exactly --steps steps once and prints BASELINE.json's metric
(`value`, `ms_per_step`, the workload in `config`); `--dump-outputs DIR` writes the detections of the last timed step as .npy files.
`--full` repeats the timed region (--repeats / --min-seconds) and adds every secondary measurement and check:
  "roofline"     : the conv stack (dominant kernel family: conv_igemm_v2_kernel / conv3x3_halo_kernel / conv_halo8_kernel /
                   conv_stem_planar_kernel / conv_head_decode_group_kernel) -- algorithmic bytes per launch / average launch
                   time, where the launch time comes from HIP events recorded on the plan's own stream around the conv
                   launches of batches that run ALONE on the GPU (one batch in flight, measured right after the timed
                   region, same process, same buffers): the number rocprofv3's kernel durations reproduce.  The in-region
                   figure (several batches sharing the GPU) and the step-time-based upper bound are reported next to it, and
                   the letterbox / post-process launches get their own HBM-roofline entries.
  "cpu_baseline" : the oracle (CPU fp32 restatement of the reference) timed on this box's host cores on a bounded sample of
                   the same workload, split into the stages of SURVEY.md 8d (transform / backbone+PAN / head / decode +
                   threshold / NMS), rank 0, N=1 only.
  "parity"       : mAP-vs-ref of the production (16-bit storage) path, and the direct checks of SURVEY.md 8d (equal counts,
                   equal labels, |dscore|, IoU) of the fp32 parity mode against the fp32 oracle.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # B/s   (MI355X_MICROARCH.md: HBM3E 8 TB/s spec)
MFMA_PEAK = 2.5e15  # FLOP/s dense fp16/bf16
# What the chip was MEASURED to deliver on this path's shapes (round 4; a secondary, labelled figure -- `roofline.frac` stays priced at the spec peaks above):
#   * matrix pipe: the vendor's tuned GEMM (hipBLASLt through torch.mm, tools/gemm_yardstick.py) reaches at most 0.99 PFLOP/s on the M x N x K of any convolution of
#     the four configs (profiles/r04a_gemm_yardstick_c5.txt, r04b_gemm_yardstick_c2.txt); an LDS-fed MFMA loop runs at a shader clock of 1.58 GHz
#     (tools/lds_mfma_bench.hip, profiles/r04j_lds_mfma_bench.txt), not the 2.4 GHz the 2.5 PFLOP/s figure assumes;
#   * memory: a device-to-device copy of a C3 canvas streams 4.99 TB/s (profiles/r02z_letterbox.txt), the best streaming kernel here 5.3 TB/s.
MFMA_MEASURED = 1.0e15
HBM_MEASURED = 5.0e12
F32_MFMA_PEAK = 157.3e12   # FLOP/s, v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: exact fp32) -- MI355X_MICROARCH.md "Matrix cores": 64 FLOP/clk/SIMD = 1/16 of the bf16 rate
F32_DEPTH = int(os.environ.get("YOLORT_AMD_F32_PIPELINE", "4"))   # plan instances of the fp32 mode at 640 x 640 (three batches in flight; 7.8 GB of fp32 activations per instance for yolov5s bs 32)

C3_SHAPES = [(1080, 1920), (720, 1280), (1920, 1080), (1080, 810), (960, 1280), (1281, 1279), (641, 480), (375, 500)]
CONFIGS = {   # BASELINE.json `configs`
    "c1": dict(arch="yolov5_darknet_pan_n_r60", dtype="fp16", batch=2, size=640, score_thresh=0.45, head_gain=0.6, shapes="fixed"),
    "c2": dict(arch="yolov5_darknet_pan_s_r60", dtype="fp16", batch=32, size=640, score_thresh=0.25, head_gain=0.4, shapes="fixed"),   # head gains: tests/test_parity_gpu.py
    "c3": dict(arch="yolov5_darknet_pan_m_r60", dtype="bf16", batch=64, size=1280, score_thresh=0.25, head_gain=2.0, shapes="dynamic"),
    "c5": dict(arch="yolov5_darknet_pan_l6_r60", dtype="fp16", batch=8, size=1280, score_thresh=0.25, head_gain=3.0, shapes="fixed"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS), help="BASELINE.json config preset (default: the headline, configs[1])")
    ap.add_argument("--arch", default=None)
    ap.add_argument("--batch", type=int, default=None, help="images per GPU per step")
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--dtype", default=None, choices=["fp16", "bf16", "fp32"],
                    help="fp32: the fp32 mode (fp32 storage + exact f32-input MFMA arithmetic: the mode that meets north_star's 1e-3 box tolerance) as a line of its own, "
                         "roofline priced at 157.3 TFLOP/s / 8 TB/s with 4-byte elements")
    ap.add_argument("--shapes", default=None, choices=["fixed", "dynamic"], help="dynamic: image sizes cycled from SURVEY 8d's list (real letterbox)")
    ap.add_argument("--score-thresh", type=float, default=None)
    ap.add_argument("--head-gain", type=float, default=None)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the CPU baseline (default: min(host cpus, 32))")
    ap.add_argument("--full", action="store_true", help="also run the secondary measurements and checks (roofline event brackets, serial / serving / dynamic-shape "
                                                            "throughput, parity, CPU baseline, --per-op) and repeat the timed region; off: the headline line alone")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write the detections of the last timed step (rank 0) to DIR/<name>.npy as float32")
    ap.add_argument("--per-op", default="", help="write a per-op profile (json) to this path after the timed run (needs --full)")
    ap.add_argument("--repeats", type=int, default=None, help="the timed region of --steps steps is run this many times back to back; value / ms_per_step are the MEDIAN repeat, "
                                                                "all repeats are reported (default: 5 with --full, else 1)")
    ap.add_argument("--min-seconds", type=float, default=None, help="keep repeating the timed region until the regions add up to this much wall time (>= --repeats regions; "
                                                                    "default: 2.0 with --full, else 0)")
    ap.add_argument("--graph", type=int, default=int(os.environ.get("YOLORT_AMD_GRAPH", "1")), help="replay the conv stack as a captured hipGraph (the package default since round 5; 0: per-kernel launches)")
    a = ap.parse_args()
    preset = CONFIGS[a.config]
    for k, v in preset.items():
        if getattr(a, k.replace("-", "_"), None) is None:
            setattr(a, k, v)
    big = a.size > 640 or a.arch.split("_")[-2] in ("m", "l", "x", "l6", "m6", "x6")
    if a.steps is None:
        a.steps = 20 if big else 60
    if a.warmup is None:
        a.warmup = 5 if big else 10
    if a.repeats is None:
        a.repeats = 5 if a.full else 1
    if a.min_seconds is None:
        a.min_seconds = 2.0 if a.full else 0.0
    if a.per_op and not a.full:
        ap.error("--per-op needs --full")
    return a


def dump_outputs(path, dets, k=300):
    """what the timed path returned for its last step, as fixed-shape float32 arrays: boxes (B, k, 4), scores (B, k), labels (B, k), zero past each
    image's count, and counts (B,)"""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    n = len(dets)
    arrs = {"boxes": np.zeros((n, k, 4), np.float32), "scores": np.zeros((n, k), np.float32), "labels": np.zeros((n, k), np.float32), "counts": np.zeros((n,), np.float32)}
    for i, d in enumerate(dets):
        m = len(d["scores"])
        arrs["counts"][i] = m
        for name in ("boxes", "scores", "labels"):
            arrs[name][i, :m] = d[name].float().cpu().numpy()
    for name, a in arrs.items():
        np.save(os.path.join(path, name + ".npy"), a)


# ----------------------------------------------------------------------------------------------------------------------
# CPU baseline (oracle = port of the reference's algorithm), stage split of SURVEY.md 8d
# ----------------------------------------------------------------------------------------------------------------------
def reference_cpu_baseline(args, sd, images_cpu, budget_s=14.0, cores=0):
    """the UNMODIFIED reference `model.predict(batch)` (yolort/models/yolov5.py:202-216) timed on the host -- possible only where /root/reference
    exists (the build container; tools/reference_cpu_baseline.py commits its figure under profiles/).  fp32 eager, torch.no_grad, 1 warm-up + timed passes; the
    stage split comes from forward hooks on transform / backbone / head (post-process = the rest).  NMS runs through oracle/_tv_compat's stand-in for
    torchvision.ops (torchvision is not installable here): reported separately inside `post_process`."""
    from oracle.reference_loader import load_reference
    load_reference()
    from yolort.models import YOLOv5 as RefYOLOv5

    host = os.cpu_count() or 1
    cores = cores or args.cpu_threads or min(host, 32)
    torch.set_num_threads(cores)
    kw = dict(size_divisible=64) if args.arch.endswith("6_r60") else {}
    model = RefYOLOv5(arch=args.arch, size=(args.size, args.size), score_thresh=args.score_thresh, nms_thresh=0.45, **kw)
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    model.eval()
    t = {"transform": 0.0, "backbone_pan": 0.0, "head": 0.0}
    marks = {}

    def pre(name):
        return lambda m, i: marks.__setitem__(name, time.perf_counter())

    def post(name):
        return lambda m, i, o: t.__setitem__(name, t[name] + time.perf_counter() - marks[name])

    for name, mod in (("transform", model.transform), ("backbone_pan", model.model.backbone), ("head", model.model.head)):
        mod.register_forward_pre_hook(pre(name))
        mod.register_forward_hook(post(name))
    imgs = [im.float() for im in images_cpu]
    with torch.no_grad():
        t0 = time.perf_counter()
        model.predict(imgs[:1])
        warm = time.perf_counter() - t0
        n_sample = int(max(1, min(len(imgs), budget_s / max(warm, 1e-3))))
        for k in t:
            t[k] = 0.0
        passes, dt, n_det = 0, 0.0, 0
        while passes < 3 and (passes == 0 or dt + dt / passes < 2 * budget_s):
            t0 = time.perf_counter()
            dets = model.predict(imgs[:n_sample])
            dt += time.perf_counter() - t0
            passes += 1
            n_det = sum(len(d["scores"]) for d in dets)
    stages = {k: round(v / (passes * n_sample) * 1e3, 2) for k, v in t.items()}
    stages["post_process"] = round((dt - sum(t.values())) / (passes * n_sample) * 1e3, 2)
    return {"value": round(passes * n_sample / dt, 3), "unit": "images/s", "cores": cores, "host_cpus": host, "kind": "reference",
            "measured_on": "build container (the only host that holds /root/reference)", "stages_ms_per_image": stages, "detections_per_image": round(n_det / n_sample, 1),
            "sample": f"{passes} pass(es) of model.predict over {n_sample} image(s) of the workload, the UNMODIFIED reference (yolort.models.YOLOv5, fp32 eager, torch CPU, "
                      f"{cores} threads); torchvision.ops.nms = oracle/_tv_compat stand-in (plain C)"}


def cpu_baseline(args, sd, images_cpu, budget_s=14.0):
    from oracle import yolov5_oracle as O
    from oracle.reference_loader import reference_available

    if reference_available():   # build container: the reference itself is the baseline (kind "reference")
        return reference_cpu_baseline(args, sd, images_cpu, budget_s)
    host = os.cpu_count() or 1
    cores = args.cpu_threads or min(host, 32)   # torch CPU convs stop scaling (and thrash) far below 256 threads
    torch.set_num_threads(cores)
    kw = dict(size_divisible=64) if args.arch.endswith("6_r60") else {}
    thr = args.score_thresh

    def staged(imgs):
        t = {}
        t0 = time.perf_counter()
        batch, _ = O.letterbox(imgs, args.size, args.size, kw.get("size_divisible", 32))
        t["transform"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        feats = O.backbone(batch, sd, "model.backbone")
        t["backbone_pan"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        ho = O.head(feats, sd, "model.head")
        t["head"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        strides, anchors = O.anchors_for(len(ho))
        pred = O.decode(ho, strides, anchors)
        cands = []
        for i in range(pred.shape[0]):   # box_head.py:414-419: scores, boxes, multi-label threshold
            p = pred[i]
            scores = p[:, 5:] * p[:, 4:5]
            cx, cy, w, h = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
            boxes = torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)
            inds, labels = torch.where(scores > thr)
            cands.append((boxes[inds], scores[inds, labels], labels))
        t["decode_threshold"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        n_c = 0
        for b, s, l in cands:            # box_head.py:422-427 (plain-C restatement of torchvision's batched_nms, oracle/nms_ref.c)
            O.batched_nms(b, s, l, 0.45)[:300]
            n_c += len(s)
        t["nms"] = time.perf_counter() - t0
        return t, n_c

    imgs = [im.float() for im in images_cpu]
    with torch.no_grad():
        t0 = time.perf_counter()
        staged(imgs[:1])                                       # warm-up (thread pool, oneDNN primitives)
        warm = time.perf_counter() - t0
        n_sample = int(max(1, min(len(imgs), budget_s / max(warm, 1e-3))))
        t0 = time.perf_counter()
        stages, n_c = staged(imgs[:n_sample])
        dt = time.perf_counter() - t0
    out = {"value": round(n_sample / dt, 3), "unit": "images/s", "cores": cores, "host_cpus": host, "kind": "port",
           "stages_ms_per_image": {k: round(v / n_sample * 1e3, 2) for k, v in stages.items()},
           "candidates_per_image": round(n_c / n_sample, 1),
           "sample": f"one pass of {n_sample} image(s) of the workload through oracle/yolov5_oracle.py (fp32, torch CPU, {cores} threads), all stages; "
                     "NMS is the oracle's plain-C restatement (single thread), not torchvision's kernel"}
    # /root/reference does not exist on this box: the UNMODIFIED reference's own timing was taken in the build container (tools/reference_cpu_baseline.py) and
    # travels as a committed record -- another host, so it is quoted beside the live port figure, labelled, never merged into it
    rpath = os.path.join(ROOT, "profiles", "reference_cpu_baseline.json")
    if os.path.exists(rpath):
        with open(rpath) as f:
            rec = json.load(f).get(args.config)
        if rec is not None:
            out["reference_on_build_container"] = rec
            out["reference_timing_measured_on"] = "build container (another host: /root/reference does not exist on the GPU box); `value` above is the oracle port timed live on this box"
    out["measured_on"] = "this box's host cores (the oracle port, live)"
    return out


# ----------------------------------------------------------------------------------------------------------------------
# parity sample
# ----------------------------------------------------------------------------------------------------------------------
from yolort_amd.utils.metrics import coco_ap  # noqa: E402  (host-side metric; re-exported for tests)


def _npd(d):
    return {"boxes": d["boxes"].detach().float().cpu().numpy(), "scores": d["scores"].detach().float().cpu().numpy(), "labels": d["labels"].detach().cpu().numpy()}


def direct_checks(ref, got, thr, k=300, score_eps=5e-4, iou_min=1 - 1e-3):
    """SURVEY.md 8d direct checks over a list of images (numpy dicts): pairs every reference detection with a HIP detection
    of the same label, |dscore| <= score_eps and IoU >= iou_min; detections within score_eps of the threshold / top-K cut may
    appear on one side only (fp32 summation order decides) and are reported as `at_cut`."""
    import numpy as np

    out = {"images": len(ref), "ref_dets": 0, "hip_dets": 0, "paired": 0, "at_cut": 0, "unexplained": 0, "images_equal_count": 0, "images_labels_equal": 0,
           "min_iou": 1.0, "max_dscore": 0.0}
    for r, g in zip(ref, got):
        rb, rs, rl, gb, gs, gl = r["boxes"], r["scores"], r["labels"], g["boxes"], g["scores"], g["labels"]
        out["ref_dets"] += len(rs)
        out["hip_dets"] += len(gs)
        out["images_equal_count"] += int(len(rs) == len(gs))
        out["images_labels_equal"] += int(len(rs) == len(gs) and bool(np.array_equal(rl, gl)))
        cut = thr
        if len(rs) >= k or len(gs) >= k:
            cut = max(thr, float(min(rs[-1] if len(rs) else 1.0, gs[-1] if len(gs) else 1.0)))
        used = np.zeros(len(gs), bool)
        for i in range(len(rs)):
            cand = np.where((gl == rl[i]) & ~used & (np.abs(gs - rs[i]) <= score_eps))[0]
            best, bj = -1.0, -1
            for j in cand:
                x1, y1 = max(rb[i, 0], gb[j, 0]), max(rb[i, 1], gb[j, 1])
                x2, y2 = min(rb[i, 2], gb[j, 2]), min(rb[i, 3], gb[j, 3])
                inter = max(x2 - x1, 0.0) * max(y2 - y1, 0.0)
                iou = inter / ((rb[i, 2] - rb[i, 0]) * (rb[i, 3] - rb[i, 1]) + (gb[j, 2] - gb[j, 0]) * (gb[j, 3] - gb[j, 1]) - inter + 1e-30)
                if iou > best:
                    best, bj = iou, j
            if bj >= 0 and best >= iou_min:
                used[bj] = True
                out["paired"] += 1
                out["min_iou"] = min(out["min_iou"], float(best))
                out["max_dscore"] = max(out["max_dscore"], abs(float(gs[bj] - rs[i])))
            elif rs[i] <= cut + score_eps:
                out["at_cut"] += 1
            else:
                out["unexplained"] += 1
        for j in np.where(~used)[0]:
            if gs[j] <= cut + score_eps:
                out["at_cut"] += 1
            else:
                out["unexplained"] += 1
    out["min_iou"] = round(out["min_iou"], 6)
    out["max_dscore"] = float(f"{out['max_dscore']:.3e}")
    return out


def conditioned_parity(args, dev, fp32_only=False):
    """The parity claim on the workload that can carry it (tests/test_golden_gpu.py): the CONDITIONED synthetic network of this architecture
    (workloads/synth.py COND_*) on its four seeded images, against detections of the UNMODIFIED reference committed as
    tests/golden/cond_<tag>.npz (made by tests/golden/make_golden.py in the build container) -- no oracle involved at run time.
      fp32 parity mode : every detection paired, same label, IoU >= 1 - 1e-3, |dscore| <= 1e-4, identical label sequences
      production 16-bit: the stated tolerance of tests/test_golden_gpu.py (TOL)"""
    import numpy as np

    from yolort_amd.models import YOLOv5
    from workloads.synth import cond_images, conditioned_weights

    from workloads.synth import spread_images

    tag = {"yolov5_darknet_pan_n_r60": "n", "yolov5_darknet_pan_s_r60": "s", "yolov5_darknet_pan_m_r60": "m", "yolov5_darknet_pan_l6_r60": "l6"}.get(args.arch)
    gold = os.path.join(ROOT, "tests", "golden")
    if tag is None or not os.path.exists(os.path.join(gold, f"cond_{tag}.npz")):
        return None
    # stated 16-bit tolerances (tests/test_golden_gpu.py); yolov5l6: none is stated -- the reference's own fp16 run pairs 6 of the golden's 27 detections -- the generous pairing is reported
    tol = {"s": (0.98, 1e-2), "l6": (0.5, 0.1), "n": (0.95, 3e-2), "m": (0.90, 6e-2)}[tag]
    spread_tol = {"s": (0.98, 1.5e-2)}.get(tag, tol)   # tests/test_golden_gpu.py SPREAD_TOL: constants, the same for every seed
    kw = dict(size_divisible=64) if args.arch.endswith("6_r60") else {}
    dt16 = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    mode_list = (("fp32_parity_mode", torch.float32),) if fp32_only else (("fp32_parity_mode", torch.float32), (f"production_{args.dtype}", dt16))
    out = {}
    # two reference-made goldens per architecture: `cond` (round 3: every score within a few hundredths of the threshold) and `spread` (round 4: scores from the threshold
    # up to ~0.9, the threshold in a gap of the reference's score list -- nothing can be excused as "at the cut").  Each also carries the REFERENCE'S OWN 16-bit run
    # (tests/golden/ref16_*.npz: the unmodified reference with .half() / .bfloat16()), the like-for-like yardstick for the production path's distance from fp32.
    import glob
    more = sorted(glob.glob(os.path.join(gold, f"spread_{tag}_s*.npz")))[:5]   # further seeds of the spread workload (make_golden.py spread-more): aggregated below
    # ... and (round 5) the LINEAR-REGIME golden: the workload on which the deep networks' 16-bit paths carry an absolute tolerance (tests/test_golden_gpu.py LIN_TOL)
    lin_tol = {("s", "fp16"): (0.98, 1e-2), ("m", "bf16"): (0.90, 2.5e-2), ("m", "fp16"): (0.98, 1e-2), ("l6", "fp16"): (0.98, 1e-2)}.get((tag, args.dtype))
    for kind, images_of, path in [("cond", cond_images, os.path.join(gold, f"cond_{tag}.npz")), ("spread", spread_images, os.path.join(gold, f"spread_{tag}.npz")),
                                  ("lin", cond_images, os.path.join(gold, f"lin_{tag}.npz"))] + [("spread", spread_images, f) for f in more]:
        if not os.path.exists(path):
            continue
        z = np.load(path)
        meta = json.loads(str(z["meta"]))
        ref = [{k: z[f"det{i}_{k}"] for k in ("boxes", "scores", "labels")} for i in range(len(meta["dets"]))]
        S, thr = meta["S"], meta["thr"]
        imgs = images_of(args.arch, meta["seed"])
        blk = {"workload": f"{kind} {args.arch}, seed {meta['seed']}, 4 seeded images of mixed shapes at {S}, thr {thr}; ground truth = detections of the UNMODIFIED reference "
                           f"(tests/golden/{os.path.basename(path)})", "reference_self_reproducibility_fp64": meta["fp64"]}
        if kind == "spread":
            blk["score_range"], blk["threshold_gap"] = meta["score_range"], meta["thr_gap"]
        for name, dtype in mode_list:
            m = YOLOv5(arch=args.arch, size=(S, S), score_thresh=thr, nms_thresh=0.45, detections_per_img=300, **kw)
            m.load_state_dict(conditioned_weights(m.state_dict(), args.arch, meta["seed"], variant=kind))
            m = m.to(dev).eval()
            m = m.set_compute_dtype(torch.float32) if dtype == torch.float32 else m.to(dtype)
            got = [_npd(d) for d in m.forward([im.to(dev) if dtype == torch.float32 else im.to(dev).to(dtype) for im in imgs])]
            if dtype == torch.float32:
                blk[name] = direct_checks(ref, got, thr, score_eps=1e-4, iou_min=1 - 1e-3)
            else:
                r16 = os.path.join(gold, "ref16_" + os.path.basename(path))
                own = json.loads(str(np.load(r16)["meta"]))[args.dtype] if os.path.exists(r16) else None
                tk = spread_tol if kind == "spread" else (lin_tol if (kind == "lin" and lin_tol is not None) else tol)
                c = direct_checks(ref, got, thr, score_eps=tk[1], iou_min=tk[0])
                relative_only = kind != "lin" and (tag == "l6" or (kind == "spread" and args.dtype == "bf16"))   # no absolute tolerance is stated there: held to the reference's OWN 16-bit run (tests/test_golden_gpu.py)
                c["stated_tolerance"] = None if relative_only else {"min_iou": tk[0], "max_dscore": tk[1]}
                c["map_vs_ref_50_95"] = coco_ap(ref, got)
                g = direct_checks(ref, got, thr, score_eps=0.1, iou_min=0.5)   # the generous pairing the reference's own 16-bit band was measured with
                c["distance_from_fp32_reference"] = {"paired": g["paired"], "of": g["ref_dets"], "iou_deficit": round(1.0 - g["min_iou"], 6), "max_dscore": g["max_dscore"]}
                if own is not None:
                    c["reference_own_" + args.dtype] = {"paired": own["paired"], "of": own["ref_dets"], "iou_deficit": own["iou_deficit"], "max_dscore": own["max_dscore"],
                                                        "what": "the UNMODIFIED reference with ." + ("half()" if args.dtype == "fp16" else "bfloat16()") + " on the same inputs vs its own fp32 detections"}
                    c["iou_deficit_vs_reference_own"] = round((1.0 - g["min_iou"]) / max(own["iou_deficit"], 1e-9), 3)
                    c["dscore_vs_reference_own"] = round(g["max_dscore"] / max(own["max_dscore"], 1e-12), 3)
                blk[name] = c
            del m
        if path in more:
            out.setdefault("spread_more_seeds", []).append(blk)
        else:
            out[kind] = blk
    if "spread_more_seeds" in out:   # one line over all further seeds: every detection of every seed counts
        per = out.pop("spread_more_seeds")
        agg = {"seeds": [int(os.path.basename(f).split("_s")[-1][:-4]) for f in more], "images": sum(b["fp32_parity_mode"]["images"] for b in per),
               "what": "further seeds of the spread workload (own weights, images and gap threshold each; same acceptance criteria as the first seed), all detections pooled"}
        for name, _dt in mode_list:
            agg[name] = {k: sum(b[name][k] for b in per) for k in ("ref_dets", "hip_dets", "paired", "at_cut", "unexplained", "images_equal_count", "images_labels_equal")}
            agg[name]["min_iou"] = min(b[name]["min_iou"] for b in per)
            agg[name]["max_dscore"] = max(b[name]["max_dscore"] for b in per)
        p16 = f"production_{args.dtype}"
        if not fp32_only and all("reference_own_" + args.dtype in b[p16] for b in per):
            agg[p16]["iou_deficit_vs_reference_own_per_seed"] = [b[p16]["iou_deficit_vs_reference_own"] for b in per]
            agg[p16]["dscore_vs_reference_own_per_seed"] = [b[p16]["dscore_vs_reference_own"] for b in per]
            agg[p16]["score_tolerance_per_seed"] = [(b[p16]["stated_tolerance"] or {}).get("max_dscore") for b in per]
            agg[p16]["reference_own_paired"] = [sum(b[p16]["reference_own_" + args.dtype]["paired"] for b in per), sum(b[p16]["reference_own_" + args.dtype]["of"] for b in per)]
        out["spread_more"] = agg
    torch.cuda.empty_cache()
    if "cond" in out:   # the round-3 layout of the block stays readable: the conditioned workload's entries at the top level
        for k, v in out["cond"].items():
            out.setdefault(k, v)
    return out


def fp32_mode_throughput(args, dev, images_cpu, steps=30, checks=None):
    """throughput of the mode that meets the north-star box tolerance (fp32 storage + exact fp32 MFMA arithmetic, csrc/conv_f32.hip) on the benchmark workload itself:
    what the tolerance costs (`only the un-benchmarked fp32 parity mode meets 1 - 1e-3`)"""
    from yolort_amd.models import YOLOv5
    from workloads.synth import synth_weights

    kw = dict(size_divisible=64) if args.arch.endswith("6_r60") else {}
    m = YOLOv5(arch=args.arch, size=(args.size, args.size), score_thresh=args.score_thresh, nms_thresh=0.45, detections_per_img=300, **kw)
    m.load_state_dict(synth_weights(m.state_dict(), args.arch, seed=0, head_gain=args.head_gain))
    m = m.to(dev).eval().set_compute_dtype(torch.float32)
    # fp32 activations are twice the size and the mode keeps every reference conv's output: at most 8 images per batch and ONE plan instance on the 1280 x 1280
    # configurations (yolov5m bs 64 in fp32 with four instances asked for 286 GiB in the first measurement set of round 4); three batches in flight at 640 x 640
    # (7.8 GB of activations per instance for yolov5s bs 32), the regime the headline is measured in
    depth = F32_DEPTH if args.size <= 640 else 1
    m.model.pipeline_depth = depth
    imgs = [im.to(dev) for im in (images_cpu if args.size <= 640 else images_cpu[:8])]

    def run(k):
        pend = []
        for _ in range(k):
            pend.append(m.forward_async(imgs))
            if len(pend) >= depth:
                pend.pop(0).result()
        for p in pend:
            p.result()

    run(2 * depth + 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    ips = len(imgs) * steps / (time.perf_counter() - t0)
    gold = bench_golden(args)
    if gold is not None and checks is not None:   # the mode that is timed here, on the timed workload, against the UNMODIFIED reference's detections (tests/golden/bench_<config>.npz)
        k = len(gold["ref"])
        got = [_npd(d) for d in m.forward(imgs[:k])]
        checks.update(direct_checks([dict(r) for r in gold["ref"]], got, args.score_thresh, score_eps=5e-4, iou_min=1 - 1e-3))
        checks["ground_truth"] = f"tests/golden/{gold['name']}"
        checks["tolerance"] = "same label, IoU >= 1 - 1e-3, |dscore| <= 5e-4; `at_cut`: within 5e-4 of the threshold / the top-300 cut on one side only"
    del m
    torch.cuda.empty_cache()
    return round(ips, 1)


def bench_golden(args):
    """the committed golden of the timed workload, when this run IS that workload: same architecture, size, threshold, head gain, fixed-size seeded images"""
    import json

    import numpy as np

    path = os.path.join(ROOT, "tests", "golden", f"bench_{args.config}.npz") if getattr(args, "config", None) else None
    if not path or not os.path.exists(path):
        return None
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    if (meta["arch"], meta["size"], meta["thr"], meta["head_gain"]) != (args.arch, args.size, args.score_thresh, args.head_gain) or args.shapes != "fixed":
        return None
    return {"name": os.path.basename(path), "meta": meta, "ref": [{k: z[f"det{i}_{k}"] for k in ("boxes", "scores", "labels")} for i in range(len(meta["dets"]))]}


def parity_sample(args, model, images_gpu, images_cpu, sd, k):
    """'mAP vs ref' of the BENCHMARK workload on a bounded sample: HIP detections scored against the oracle's as ground truth.
    This workload (U[0,1) noise images, BN gamma ~ 1, ~1000 near-tied candidates per image, 300 kept) is the throughput workload -- it stresses
    the post-process -- and cannot carry a tight tolerance: a rounding is amplified ~2500x on its way to the logits;
    the parity CLAIM is `conditioned_parity` above."""
    import numpy as np

    from oracle import yolov5_oracle as O

    kw = dict(size_divisible=64) if args.arch.endswith("6_r60") else {}
    thr = args.score_thresh
    # round 6: when the timed workload has a committed golden (tests/golden/bench_<config>.npz: detections of the UNMODIFIED reference on exactly these weights and
    # images, tests/golden/make_golden.py bench), the ground truth is the reference itself, not the oracle
    gold = bench_golden(args)
    if gold is not None:
        k = min(k, len(gold["ref"]))
    cpu = [im.float() for im in images_cpu[:k]]
    dt16 = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    with torch.no_grad():
        ref = gold["ref"][:k] if gold is not None else O.yolov5_forward(cpu, sd, size=(args.size, args.size), score_thresh=thr, **kw)
        emu = None
        if args.size <= 640:
            # the same oracle with 16-bit STORAGE emulated between layers (fp32 arithmetic): what any 16-bit-storage implementation
            # can expect against the fp32 reference on this network -- the yardstick for the production path's own figure
            O.EMULATE.dtype = dt16
            try:
                emu = O.yolov5_forward([im.to(dt16).float() for im in cpu], sd, size=(args.size, args.size), score_thresh=thr, **kw)
            finally:
                O.EMULATE.dtype = None
    got = model.forward(images_gpu[:k])
    refs, gots = ([dict(r) for r in ref] if gold is not None else [_npd(r) for r in ref]), [_npd(d) for d in got]
    ious, matched, total = [], 0, 0
    for r, d in zip(refs, gots):
        total += len(r["labels"])
        for i in range(len(r["labels"])):
            c = np.where(d["labels"] == r["labels"][i])[0]
            if len(c) == 0:
                continue
            rb, gb = r["boxes"], d["boxes"]
            x1, y1 = np.maximum(rb[i, 0], gb[c, 0]), np.maximum(rb[i, 1], gb[c, 1])
            x2, y2 = np.minimum(rb[i, 2], gb[c, 2]), np.minimum(rb[i, 3], gb[c, 3])
            inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
            iou = inter / ((rb[i, 2] - rb[i, 0]) * (rb[i, 3] - rb[i, 1]) + (gb[c, 2] - gb[c, 0]) * (gb[c, 3] - gb[c, 1]) - inter + 1e-12)
            best = float(iou.max())
            if best >= 0.5:
                matched += 1
                ious.append(best)
    ap = coco_ap(refs, gots)
    out = {"images": k, "ref_dets": total, "matched_iou50": round(matched / max(total, 1), 4),
           "median_iou": round(float(np.median(ious)), 4) if ious else None,
           "map_vs_ref_50_95": round(ap, 4) if ap is not None else None,
           "ground_truth": (f"tests/golden/{gold['name']}: detections of the UNMODIFIED reference on this workload (make_golden.py bench)" if gold is not None
                            else "oracle (fp32 CPU restatement of the reference)"),
           "note": f"benchmark (saturated noise-image) workload; the production path stores {args.dtype}"}
    if gold is not None:   # the direct checks of SURVEY.md 8d of the production path against the reference at the tolerance the conditioned goldens carry for 16-bit storage
        out["direct_checks_iou98_ds1e-2"] = direct_checks(refs, gots, thr, score_eps=1e-2, iou_min=0.98)
    if emu is not None:
        ap_emu = coco_ap(refs, [_npd(r) for r in emu])
        out["map_of_oracle_with_emulated_16bit_storage"] = round(ap_emu, 4) if ap_emu is not None else None
    return out


def _elapsed(pairs):
    return [s.elapsed_time(t) for s, t in zip(*pairs)]


def main_fp32(args):
    """`--dtype fp32`: the fp32 mode as a bench line of its own.  Same step, same workload, same timing contract as the headline; the model keeps
    fp32 parameters, activations are stored in fp32 and every convolution is exact fp32 arithmetic on v_mfma_f32_32x32x2_f32 (csrc/conv_f32_pipe.hip) -- the arithmetic of
    the reference's CPU path (common.py:69-70 in torch.float32).  Roofline: per-launch bound max(flops / 157.3 TFLOP/s, bytes / 8 TB/s) at 4 bytes per element."""
    if int(os.environ.get("WORLD_SIZE", "1")) != 1 or args.gpus != 1:
        raise SystemExit("--dtype fp32 is a single-GPU line (the sharded path is dtype-agnostic: run the default dtype with --gpus N)")
    dev = torch.device("cuda", int(os.environ.get("YOLORT_AMD_BENCH_DEVICE", "0")))
    torch.cuda.set_device(dev)
    from yolort_amd.models import YOLOv5
    from workloads.synth import synth_images, synth_weights

    kw = dict(size_divisible=64) if args.arch.endswith("6_r60") else {}
    model = YOLOv5(arch=args.arch, size=(args.size, args.size), score_thresh=args.score_thresh, nms_thresh=0.45, detections_per_img=300, **kw)
    sd = synth_weights(model.state_dict(), args.arch, seed=0, head_gain=args.head_gain)
    model.load_state_dict(sd)
    model = model.to(dev).eval().set_compute_dtype(torch.float32)
    if args.shapes == "dynamic":
        images_cpu = [synth_images(1, *C3_SHAPES[i % len(C3_SHAPES)], seed=1 + i)[0] for i in range(args.batch)]
    else:
        images_cpu = list(synth_images(args.batch, args.size, args.size, seed=1))
    images_gpu = [im.to(dev) for im in images_cpu]
    yolo = model.model
    yolo.pipeline_depth = int(os.environ.get("YOLORT_AMD_PIPELINE", str(F32_DEPTH if args.size <= 640 else 1)))
    depth = max(1, yolo.pipeline_depth - 1)
    host = {"enqueue": 0.0}

    def run_steps(k):
        pending, dets = [], None
        for _ in range(k):
            t_a = time.perf_counter()
            pending.append(model.forward_async(images_gpu))
            host["enqueue"] += time.perf_counter() - t_a
            if len(pending) > depth:
                dets = pending.pop(0).result()
        while pending:
            dets = pending.pop(0).result()
        return dets

    run_steps(max(args.warmup, 1))
    torch.cuda.synchronize()
    e = next(iter(yolo._entries.values()))

    def timed_region():
        torch.cuda.synchronize()
        host["enqueue"] = 0.0
        t0 = time.perf_counter()
        d = run_steps(args.steps)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, host["enqueue"] / args.steps * 1e3, d

    reps = [timed_region()]
    reps += [timed_region() for _ in range(min(400, max(1, args.repeats, int(args.min_seconds / max(reps[0][0], 1e-6)) + 1)) - 1)]
    order = sorted(range(len(reps)), key=lambda i: reps[i][0])
    elapsed, host_enqueue_ms, dets = reps[order[len(order) // 2]]
    rep_ips = [round(args.batch * args.steps / r[0], 1) for r in reps]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, reps[-1][2])
    step_s = elapsed / args.steps
    ips = args.batch * args.steps / elapsed
    conv_meta = [m for m in e.plan.meta if m["kind"] == "conv"]
    n_conv = len(conv_meta)
    tiles = {}
    for m in conv_meta:
        tiles[str(m.get("tile"))] = tiles.get(str(m.get("tile")), 0) + 1
    out = {
        "metric": ("images/sec at 640x640 (bs=32) yolov5s" if args.config == "c2" else f"images/sec at {args.size}x{args.size} (bs={args.batch}) {args.arch}") + " -- fp32 mode",
        "value": round(ips, 2), "unit": "images/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(step_s * 1e3, 4),
        "repeats": {"n": len(reps), "images_per_s": rep_ips if len(rep_ips) <= 12 else rep_ips[:4] + ["..."] + rep_ips[-4:], "median": round(ips, 2), "min": min(rep_ips), "max": max(rep_ips),
                    "spread_pct": round(100.0 * (max(rep_ips) - min(rep_ips)) / max(ips, 1e-9), 2), "timed_seconds_total": round(sum(r[0] for r in reps), 3)},
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{args.arch} fp32 mode (fp32 storage, exact fp32 arithmetic on the f32-input MFMA) bs={args.batch}/GPU {args.size}x{args.size} "
                               + ("dynamic-shape letterbox (8 cycled sizes, SURVEY 8d)" if args.shapes == "dynamic" else "fixed-size stream (letterbox kernel: planar fp32 -> NHWC4 canvas)")
                               + " -> backbone+PAN+head -> decode+NMS HIP path", "score_thresh": args.score_thresh, "nms_thresh": 0.45, "detections_per_img": 300,
                   "weights": f"seeded synthetic (workloads/synth.py, head_gain {args.head_gain})", "batches_in_flight": depth, "plan_instances": yolo.pipeline_depth,
                   "host_enqueue_ms_per_step_rank0": round(host_enqueue_ms, 4), "canvas": [e.x.h, e.x.w], "detections_per_step_rank0": int(sum(len(d["scores"]) for d in dets)),
                   "conv_tiles": tiles, "plan_activation_bytes": e.plan.bytes_allocated},
    }
    if not args.full:
        print(json.dumps(out))
        return
    # the conv launches with ONE batch in flight: HIP events on the stream they are launched on
    yolo.bracket = {"pre": ([], []), "conv": ([], []), "post": ([], [])}
    n_excl = 6
    for _ in range(n_excl):
        model.forward_async(images_gpu).result()
        torch.cuda.synchronize()
    excl = {k: _elapsed(v) for k, v in yolo.bracket.items()}
    yolo.bracket = None
    mean = lambda v: (sum(v) / len(v)) if v else 0.0  # noqa: E731
    bytes_step, flops_step = sum(m["bytes"] for m in conv_meta), sum(m["flops"] for m in conv_meta)
    bound_s = sum(max(m["flops"] / F32_MFMA_PEAK, m["bytes"] / HBM_PEAK) for m in conv_meta)
    n_mfma_bound = sum(1 for m in conv_meta if m["flops"] / F32_MFMA_PEAK >= m["bytes"] / HBM_PEAK)
    conv_s = mean(excl["conv"]) * 1e-3
    # HBM traffic of the fp32 conv launches from the committed PMC passes (rocprofv3 cannot run inside this process): per launch like `achieved`; only for the workload it was measured on
    traffic = None
    tpath = os.path.join(ROOT, "profiles", "conv_traffic_fp32.json")
    if os.path.exists(tpath) and args.config == "c2" and args.arch == CONFIGS["c2"]["arch"] and args.batch == 32 and args.size == 640:
        with open(tpath) as f:
            tj = json.load(f)
        if "fetch_mb_per_step_corrected" in tj:
            tb = (tj["fetch_mb_per_step_corrected"] + tj["write_mb_per_step"]) * 1e6
            traffic = {"bytes_per_launch": round(tb / max(n_conv, 1)), "bytes_per_step": round(tb), "vs_algorithmic": round(tb / max(bytes_step, 1), 3),
                       "source": "profiles/conv_traffic_fp32.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, tools/profile_serial.py --config c2 --fp32)", "correction": tj.get("correction")}
    out["roofline"] = {"bound": "mfma", "achieved": round(flops_step / conv_s / 1e12, 2) if conv_s > 0 else 0.0, "peak": F32_MFMA_PEAK / 1e12, "unit": "TFLOP/s",
                       "frac": round(bound_s / conv_s, 4) if conv_s > 0 else 0.0,
                       "frac_definition": f"per-launch bound sum_l max(flops_l / 157.3 TFLOP/s, bytes_l / 8 TB/s) at 4 bytes per element / measured serial conv time; {n_mfma_bound} of {n_conv} launches are MFMA-bound",
                       "frac_mfma": round(flops_step / conv_s / F32_MFMA_PEAK, 4) if conv_s > 0 else 0.0, "traffic": traffic,
                       "kernel": "conv_f32_pipe_kernel (every conv launch of one step; csrc/conv_f32_pipe.hip)", "launches_per_step": n_conv,
                       "algorithmic_flops_per_step": flops_step, "algorithmic_bytes_per_step": bytes_step, "algorithmic_flops_per_launch": round(flops_step / max(n_conv, 1)),
                       "per_layer_bound_ms": round(bound_s * 1e3, 4),
                       "serial": {"conv_ms_per_step": round(conv_s * 1e3, 4), "avg_launch_us": round(conv_s / max(n_conv, 1) * 1e6, 2),
                                  "timing": f"HIP events on the plan's stream around the conv launches, one batch in flight, mean of {n_excl} steps right after the timed region"},
                       "pipelined": {"batches_in_flight": depth, "ms_per_step": round(step_s * 1e3, 4), "frac_of_per_layer_bound": round(bound_s / step_s, 4),
                                     "tflops": round(flops_step / step_s / 1e12, 2)},
                       "other_kernels": {"letterbox": {"ms": round(mean(excl["pre"]), 4)} if excl["pre"] else None, "postprocess": {"ms": round(mean(excl["post"]), 4)} if excl["post"] else None}}
    if not args.no_cpu_baseline:
        sd_cpu = {k: v.float().cpu() for k, v in model.state_dict().items()}
        cp = conditioned_parity(args, dev, fp32_only=True)
        out["parity"] = {} if cp is None else dict(cp)
        if cp is not None:
            out["parity"]["unexplained"] = sum(cp[k]["fp32_parity_mode"]["unexplained"] for k in ("cond", "spread", "spread_more", "lin") if k in cp)
            out["parity"]["north_star_tolerance"] = "boxes within 1e-3 IoU, |dscore| <= 1e-4, identical label sequences against detections of the UNMODIFIED reference (tests/golden/*.npz)"
        out["cpu_baseline"] = cpu_baseline(args, sd_cpu, images_cpu)
    print(json.dumps(out))


def main():
    args = parse()
    if args.dtype == "fp32":
        return main_fp32(args)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit(f"--gpus {args.gpus} needs a torch.distributed.run launch with --nproc-per-node {args.gpus}")
    dev_index = int(os.environ.get("YOLORT_AMD_BENCH_DEVICE", local_rank))   # default: one GPU per rank (LOCAL_RANK)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("YOLORT_AMD_BENCH_BACKEND", "nccl")   # "nccl" IS RCCL on ROCm; "gloo" only for the two-ranks-on-one-GPU control-flow test
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from yolort_amd import dist as ydist
    from yolort_amd.models import YOLOv5
    from workloads.synth import synth_images, synth_weights

    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    kw = dict(size_divisible=64) if args.arch.endswith("6_r60") else {}
    model = YOLOv5(arch=args.arch, size=(args.size, args.size), score_thresh=args.score_thresh, nms_thresh=0.45, detections_per_img=300, **kw)
    sd = synth_weights(model.state_dict(), args.arch, seed=0, head_gain=args.head_gain)
    model.load_state_dict(sd)
    model = model.to(dev).to(dtype).eval()

    # each rank's shard of the (weak-scaled) global batch: seeds differ per rank
    if args.shapes == "dynamic":
        images_cpu = [synth_images(1, *C3_SHAPES[i % len(C3_SHAPES)], seed=1 + rank * 1000 + i)[0] for i in range(args.batch)]
    else:
        images_cpu = list(synth_images(args.batch, args.size, args.size, seed=1 + rank))
    images_gpu = [im.to(dev).to(dtype) for im in images_cpu]

    yolo = model.model
    yolo.use_graph = bool(args.graph)
    yolo.pipeline_depth = int(os.environ.get("YOLORT_AMD_PIPELINE", "4"))

    # serving loop with `depth` batches in flight: submit batch i+depth, then collect batch i.  Each plan
    # instance owns a conv stream and a post-process stream, so consecutive batches overlap on the GPU and
    # the host-side result handling is hidden.  Every submitted batch is collected inside the timed region.
    depth = max(1, yolo.pipeline_depth - 1)   # batches in flight before the oldest is collected

    gather_on, second_rounds = [False], [0]

    def collect(p):
        dets = p.result()
        if gather_on[0]:
            p.gathered()   # every rank, every batch, in submission order: collective when some rank re-ran the batch (dist.resolve_stale)
            second_rounds[0] += int(p.second_round)
        return dets

    host = {"enqueue": 0.0, "collect": 0.0}   # host-side seconds spent submitting / collecting (the rest of a step the host waits for the GPU)

    def run_steps(k):
        pending, dets = [], None
        for _ in range(k):
            t_a = time.perf_counter()
            pending.append(model.forward_async(images_gpu))
            host["enqueue"] += time.perf_counter() - t_a
            if len(pending) > depth:
                dets = collect(pending.pop(0))
        while pending:
            dets = collect(pending.pop(0))
        return dets

    if world > 1:
        run_steps(1)                       # plan build and the first candidate-capacity growth happen locally, before the gather is on
        yolo.enable_distributed_gather()   # the slab all-gather is enqueued behind each batch's post-process (no host sync before it)
        gather_on[0] = True

    dets = run_steps(max(args.warmup, 1))
    torch.cuda.synchronize()
    e = next(iter(yolo._entries.values()))
    yolo.bracket = None   # the timed regions run the product's default submit path (two C-ABI calls per batch); the event brackets get a region of their own below

    if world > 1:
        import torch.distributed as dist

    def timed_region():
        """EXACTLY args.steps steps between barrier + synchronize on both sides; the maximum over ranks"""
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        host["enqueue"] = 0.0
        t0 = time.perf_counter()
        d = run_steps(args.steps)
        enq = host["enqueue"] / args.steps * 1e3
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, enq, d

    # the region is run `repeats` times back to back (a 20-step region is 26 ms: one sample says little on a pool whose boxes and clocks wander by +-5 %);
    # value / ms_per_step / host_enqueue are the MEDIAN repeat's, every repeat is in the line
    # The region (EXACTLY --steps steps) is repeated back to back: at least --repeats times and until the regions hold >= --min-seconds of GPU work (a 60-step region of the
    # headline is 73 ms: five of them say little on a pool whose clocks settle over seconds, and the driver's gpu_busy sampler sees nothing -- VERDICT r4 weak 10).
    # value / ms_per_step / host_enqueue are the MEDIAN region's; the spread over all regions is in the line.  The number of regions is agreed across ranks.
    reps = [timed_region()]
    n_reg = max(1, args.repeats, int(args.min_seconds / max(reps[0][0], 1e-6)) + 1)
    n_reg = min(n_reg, 400)
    if world > 1:
        t_n = torch.tensor([n_reg], device=dev, dtype=torch.int64)
        dist.all_reduce(t_n, op=dist.ReduceOp.MAX)
        n_reg = int(t_n.item())
    reps += [timed_region() for _ in range(n_reg - 1)]
    order = sorted(range(len(reps)), key=lambda i: reps[i][0])
    elapsed, host_enqueue_ms, dets = reps[order[len(order) // 2]]
    rep_ips = [round(world * args.batch * args.steps / r[0], 1) for r in reps]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, reps[-1][2])
    step_s = elapsed / args.steps
    ips = world * args.batch * args.steps / elapsed
    out = None
    if rank == 0:
        workload = (f"{args.arch} {args.dtype} bs={args.batch}/GPU {args.size}x{args.size} "
                    + ("dynamic-shape letterbox (8 cycled sizes, SURVEY 8d) -> " if args.shapes == "dynamic" else "fixed-size stream (letterbox = identity: the stem reads the planar images) -> ")
                    + f"backbone+PAN+head+decode+NMS HIP path (BASELINE configs[{dict(c1=0, c2=1, c3=2, c5=4)[args.config]}])")
        out = {
            "metric": "images/sec at 640x640 (bs=32) yolov5s" if args.config == "c2" else f"images/sec at {args.size}x{args.size} (bs={args.batch}) {args.arch}",
            "value": round(ips, 2),
            "unit": "images/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(step_s * 1e3, 4),
            "repeats": {"n": len(reps), "images_per_s": rep_ips if len(rep_ips) <= 12 else rep_ips[:4] + ["..."] + rep_ips[-4:], "median": round(ips, 2), "min": min(rep_ips), "max": max(rep_ips),
                        "spread_pct": round(100.0 * (max(rep_ips) - min(rep_ips)) / max(ips, 1e-9), 2),
                        "p10_p90": [sorted(rep_ips)[len(rep_ips) // 10], sorted(rep_ips)[(9 * len(rep_ips)) // 10 - (1 if len(rep_ips) >= 10 else 0)]],
                        "timed_seconds_total": round(sum(r[0] for r in reps), 3),
                        "note": "the timed region (exactly `steps` steps, barrier + synchronize on both sides) run back to back until >= --min-seconds of work; value / ms_per_step are the median region"},
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {"workload": workload, "score_thresh": args.score_thresh, "nms_thresh": 0.45, "detections_per_img": 300,
                       "weights": f"seeded synthetic (workloads/synth.py, head_gain {args.head_gain})", "parallelism": f"dp{world} (one shard per rank, slab all-gather)",
                       "gather_second_rounds_rank0": second_rounds[0], "host_enqueue_ms_per_step_rank0": round(host_enqueue_ms, 4),
                       "submit_path_of_timed_regions": ("ymi_plan_begin + ymi_plan_submit (the product's default: two C-ABI calls per batch, conv stack and post-process as one graph launch each)"
                                                        if world == 1 else "torch-level sequence (the slab all-gather is enqueued from Python behind each batch)"),
                       "canvas": [e.x.h, e.x.w], "detections_per_step_rank0": int(sum(len(d["scores"]) for d in dets)),
                       "conv_tiles": "pinned table yolort_amd/data/tiles_gfx950.json" if not e.plan.autotune else "autotuned at plan build"},
        }
    if not args.full:
        if rank == 0:
            print(json.dumps(out))
        if world > 1:
            dist.destroy_process_group()
        return
    # one more region, NOT part of `value`: event pairs recorded on the launching streams around each batch's conv / post-process launches while batches overlap (the
    # brackets take the torch-level submit sequence: 0.05 ms more host time per batch than the default path -- which is why they are no longer inside the timed regions)
    yolo.bracket = {"pre": ([], []), "conv": ([], []), "post": ([], [])}
    timed_region()
    region = {k: _elapsed(v) for k, v in yolo.bracket.items()}
    # the SERIAL regime as a throughput: one batch in flight, every batch collected before the next is submitted (what a latency-bound caller sees)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        collect(model.forward_async(images_gpu))
    torch.cuda.synchronize()
    serial_ips = world * args.batch * args.steps / (time.perf_counter() - t0)
    # the same launches with ONE batch in flight (no overlap with other batches' kernels), right after the timed region:
    # per-launch durations as rocprofv3 sees them.  The in-region brackets above include the time a batch's kernels share
    # the GPU with the neighbouring batches' conv / post-process kernels.
    yolo.bracket = {"pre": ([], []), "conv": ([], []), "post": ([], [])}
    n_excl = 10
    # the shader clock while the conv stack runs (s_memtime cycles per 100 MHz tick, one idle wave on a side stream: ymi_clock_probe)
    clock_mhz = None
    try:
        from yolort_amd import _lib as ylib
        probe = torch.zeros(2, dtype=torch.int64, device=dev)
        side = torch.cuda.Stream(device=dev)
        ylib.check(ylib.load().ymi_clock_probe(probe.data_ptr(), 4000, ylib.stream_ptr(side)), "ymi_clock_probe")
    except Exception:
        probe = None
    for _ in range(n_excl):
        last = model.forward_async(images_gpu)
        collect(last)
        torch.cuda.synchronize()
    # candidate counts of the TIMED workload, read from the status words of its own last batch before anything else runs (status[4]: every (anchor, class) pair above
    # the threshold; status[0]: the records that were sorted after the score-prefix selection -- round 3 reported the latter, of whatever batch ran last, as "candidates")
    st_words = last.entry.post.status.tolist() if last.entry.post is not None else [0] * 8
    n_cand_raw, n_cand_sorted = int(st_words[4]), int(st_words[0])
    if probe is not None:
        torch.cuda.synchronize()
        cyc, ticks = [int(v) for v in probe.tolist()]
        clock_mhz = round(cyc / max(ticks, 1) * 100.0, 1)
    excl = {k: _elapsed(v) for k, v in yolo.bracket.items()}
    yolo.bracket = None
    mean = lambda v: (sum(v) / len(v)) if v else 0.0  # noqa: E731
    # the host's submit path in SERVING mode (frozen weights + the conv stack as one hipGraph launch): a secondary measurement, the headline runs the defaults
    serving = None
    if rank == 0 and world == 1:
        g0 = yolo.use_graph
        model.freeze_weights(True)
        yolo.use_graph = True
        run_steps(3)
        torch.cuda.synchronize()
        host["enqueue"] = 0.0
        t0 = time.perf_counter()
        run_steps(args.steps)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        serving = {"host_enqueue_ms_per_step": round(host["enqueue"] / args.steps * 1e3, 4), "images_per_s": round(args.batch * args.steps / el, 1),
                   "mode": "YOLOv5.freeze_weights() + hipGraph replay of the conv stack (YOLORT_AMD_GRAPH=1)"}
        model.freeze_weights(False)
        yolo.use_graph = g0
    dyn = None
    if rank == 0 and world == 1 and args.shapes == "fixed" and not args.no_cpu_baseline:
        # secondary measurement ("<config>dyn"): the same model on a stream of the 8 cycled image sizes of SURVEY 8d, scaled to this config's
        # size -- a fixed-size stream never runs the letterbox kernel (the stem reads the planar images), so its HBM figure comes from here
        sc = args.size / 1280.0
        dyn_cpu = [synth_images(1, max(32, int(h * sc)), max(32, int(w * sc)), seed=7000 + i)[0] for i, (h, w) in enumerate(C3_SHAPES * ((args.batch + 7) // 8))][: args.batch]
        dyn_gpu = [im.to(dev).to(dtype) for im in dyn_cpu]
        for _ in range(3):
            collect(model.forward_async(dyn_gpu))
        torch.cuda.synchronize()
        yolo.bracket = {"pre": ([], []), "conv": ([], []), "post": ([], [])}
        for _ in range(n_excl):
            collect(model.forward_async(dyn_gpu))
            torch.cuda.synchronize()
        ex2 = {k: _elapsed(v) for k, v in yolo.bracket.items()}
        yolo.bracket = None
        # ... and its throughput in the regime `value` is measured in (batches in flight, letterbox launch included)
        dyn_steps = max(10, args.steps // 2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pend = []
        for _ in range(dyn_steps):
            pend.append(model.forward_async(dyn_gpu))
            if len(pend) > depth:
                collect(pend.pop(0))
        while pend:
            collect(pend.pop(0))
        torch.cuda.synchronize()
        dyn_ips = args.batch * dyn_steps / (time.perf_counter() - t0)
        in_b = sum(im.numel() * im.element_size() for im in dyn_gpu)
        hb, wb = e.x.h, e.x.w   # portrait and landscape shapes in one batch: the canvas is the full size x size square, the fixed stream's own plan
        if ex2["pre"]:
            ms = mean(ex2["pre"])
            lbb = in_b + args.batch * hb * wb * 4 * 2
            dyn = {"workload": f"{args.config}dyn: the same model, bs {args.batch}, the 8 cycled image sizes of SURVEY 8d scaled by {sc:g} -> canvas {hb}x{wb}",
                   "letterbox_tile2_kernel": {"ms": round(ms, 4), "algorithmic_bytes": lbb, "achieved_GBps": round(lbb / ms / 1e6, 1), "frac_of_hbm_peak": round(lbb / (ms * 1e-3) / HBM_PEAK, 4)},
                   "conv_ms_per_step_serial": round(mean(ex2["conv"]), 4), "images_per_s": round(dyn_ips, 1), "steps": dyn_steps}

    if rank == 0:
        conv_meta = [m for m in e.plan.meta if m["kind"] == "conv"]
        n_conv = len(conv_meta) - (1 if (e.plan.stem_body1_fusable() and (args.shapes == "fixed" or e.plan.fuse_stem)) else 0)   # stem + body.1 run as one launch
        bytes_step = sum(m["bytes"] for m in conv_meta)
        flops_step = sum(m["flops"] for m in conv_meta)
        # one bound per REFERENCE conv: a launch that stands for several (the strip kernel, engine.Plan.c3_tile) carries them as `layers`
        per_layer = [fb for m in conv_meta for fb in (m.get("layers") or [(m["flops"], m["bytes"])])]
        bound_s = sum(max(f / MFMA_PEAK, b / HBM_PEAK) for f, b in per_layer)
        bound_meas_s = sum(max(f / MFMA_MEASURED, b / HBM_MEASURED) for f, b in per_layer)
        conv_s = mean(excl["conv"]) * 1e-3                 # serial duration of the conv launches of one step
        conv_s_region = mean(region["conv"]) * 1e-3
        achieved = bytes_step / conv_s / 1e9 if conv_s > 0 else 0.0
        # HBM traffic of the conv launches from the committed PMC passes (rocprofv3 cannot run inside this process):
        # per launch like `achieved`; only quoted for the workload it was measured on
        traffic = None
        tpath = os.path.join(ROOT, "profiles", "conv_traffic.json")
        if os.path.exists(tpath) and args.config == "c2" and args.arch == CONFIGS["c2"]["arch"] and args.batch == 32 and args.size == 640 and args.dtype == "fp16":
            with open(tpath) as f:
                tj = json.load(f)
            traffic = {"bytes_per_launch": round((tj["fetch_mb_per_step_corrected"] + tj["write_mb_per_step"]) * 1e6 / max(n_conv, 1)),
                       "bytes_per_step": round((tj["fetch_mb_per_step_corrected"] + tj["write_mb_per_step"]) * 1e6), "source": tj["source"], "correction": tj["correction"]}
        # HBM-bound edge kernels: algorithmic bytes / exclusive event time
        n_cand = n_cand_raw
        in_bytes = sum(im.numel() * im.element_size() for im in images_gpu)
        lb_bytes = in_bytes + args.batch * e.x.h * e.x.w * 4 * 2
        kernels = {}
        if excl["pre"]:
            ms = mean(excl["pre"])
            kernels["letterbox_tile2_kernel"] = {"ms": round(ms, 4), "algorithmic_bytes": lb_bytes, "achieved_GBps": round(lb_bytes / ms / 1e6, 1),
                                           "frac_of_hbm_peak": round(lb_bytes / (ms * 1e-3) / HBM_PEAK, 4), "launches_per_step": (args.batch + 63) // 64}
        if excl["post"]:
            ms = mean(excl["post"])
            pbytes = n_cand * 12 + n_cand_sorted * 12 * 3 + args.batch * e.post.total_anchors * 16   # every record read once by the selection, the selected ones by rank / scatter / NMS + the boxes of every anchor
            kernels["postprocess (select_prefix + sort_image + nms_segments + gather_topk)"] = {
                "ms": round(ms, 4), "candidates_per_step": n_cand, "records_sorted_per_step": n_cand_sorted, "algorithmic_bytes": pbytes, "achieved_GBps": round(pbytes / ms / 1e6, 1),
                "frac_of_hbm_peak": round(pbytes / (ms * 1e-3) / HBM_PEAK, 5), "note": "latency-bound (per-image sort + greedy NMS), not bandwidth-bound"}
        out["serial_images_per_s"] = round(serial_ips, 1)
        out["config"].update({"gather_second_rounds_rank0": second_rounds[0], "serving_mode_rank0": serving,
                              "candidates_per_step_rank0": n_cand, "records_sorted_per_step_rank0": n_cand_sorted})
        # `frac` is the PER-LAYER fraction SURVEY.md 8d prescribes (sum over the conv launches of max(flops / MFMA peak, bytes / HBM peak),
        # divided by the measured conv time) in the SERIAL regime; achieved / peak / frac_hbm are the plain bytes-over-time view of the
        # same measurement.  The two regimes are spelled out: `serial` = one batch in flight (what rocprofv3's kernel durations add up
        # to); `pipelined` = the timed region, `batches_in_flight` batches on separate streams filling each other's launch gaps and
        # partial waves -- the regime `value` is measured in (its step time also holds the letterbox / post-process launches).
        out["roofline"] = {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                           "frac": round(bound_s / conv_s, 4) if conv_s > 0 else 0.0,
                           "frac_definition": "per-layer bound (SURVEY 8d): sum_l max(flops_l / 2.5 PFLOP/s, bytes_l / 8 TB/s) / measured serial conv time; 49 of 60 yolov5s layers are HBM-bound",
                           "frac_hbm": round(achieved * 1e9 / HBM_PEAK, 4),
                           "against_measured_ceilings": {"mfma_tflops": MFMA_MEASURED / 1e12, "hbm_gbps": HBM_MEASURED / 1e9, "per_layer_bound_ms": round(bound_meas_s * 1e3, 4),
                                                         "frac": round(bound_meas_s / conv_s, 4) if conv_s > 0 else 0.0,
                                                         "note": "the same per-layer bound priced at what this chip was measured to deliver on these shapes (vendor GEMM <= 0.99 PFLOP/s, "
                                                                 "copy 5 TB/s; shader clock 1.58 GHz under LDS + MFMA load) -- context, not the contract's fraction"},
                           "traffic": traffic,
                           "kernel": "conv family: c3_tile_kernel (the C3 strip kernel: 8 of the 29 launches, 39 % of the time), conv_igemm_v2_kernel, conv_igemm8_kernel, conv_halo8_kernel, conv3x3_rs_kernel, c3_fused32_kernel, stem_body1_fused_kernel, conv_head_decode_group_kernel (all conv launches of one step)",
                           "shader_clock_mhz_measured": clock_mhz,
                           "peaks_priced_at": "2.4 GHz (2.5 PFLOP/s dense fp16 / bf16) and 8 TB/s, as the contract demands; the chip sustains the measured clock under this load",
                           "launches_per_step": n_conv, "algorithmic_bytes_per_step": bytes_step, "algorithmic_bytes_per_launch": round(bytes_step / max(n_conv, 1)),
                           "algorithmic_flops_per_step": flops_step, "per_layer_bound_ms": round(bound_s * 1e3, 4),
                           "serial": {"conv_ms_per_step": round(conv_s * 1e3, 4), "avg_launch_us": round(conv_s / max(n_conv, 1) * 1e6, 2),
                                      "frac_of_per_layer_bound": round(bound_s / conv_s, 4) if conv_s > 0 else 0.0, "frac_of_hbm_peak": round(achieved * 1e9 / HBM_PEAK, 4),
                                      "tflops": round(flops_step / conv_s / 1e12, 2) if conv_s > 0 else 0.0,
                                      "timing": f"HIP events on the plan's stream around the conv launches, one batch in flight, mean of {n_excl} steps right after the timed region"},
                           "pipelined": {"batches_in_flight": depth, "ms_per_step": round(step_s * 1e3, 4),
                                         "frac_of_per_layer_bound": round(bound_s / step_s, 4), "frac_of_hbm_peak": round(bytes_step / step_s / HBM_PEAK, 4),
                                         "tflops": round(flops_step / step_s / 1e12, 2),
                                         "conv_bracket_ms": round(conv_s_region * 1e3, 4),
                                         "conv_bracket_submit_path": "torch-level sequence with event pairs, in a region of its own that is not part of `value`",
                                         "note": "per-layer bound / ms_per_step of the timed region: a LOWER bound on the conv stack's fraction there (the step also holds the "
                                                 "post-process launches); conv_bracket_ms = event brackets around one batch's conv launches while they share the GPU with its neighbours' kernels"},
                           "other_kernels": kernels}
        if dyn is not None:
            out["roofline"]["other_kernels"]["dynamic_shape_stream"] = dyn
            # secondary value: the same model on the dynamic-shape stream -- every batch runs the letterbox launch (the headline stream is letterbox-free: its
            # images already are the canvas and the stem reads them directly)
            out["secondary"] = {f"{args.config}dyn_images_per_s": dyn["images_per_s"], "workload": dyn["workload"]}
        if world == 1 and not args.no_cpu_baseline:
            sd_cpu = {k: v.float().cpu() for k, v in model.state_dict().items()}
            k_par = 4 if args.size <= 640 else 2
            cp = conditioned_parity(args, dev)
            out["parity"] = {} if cp is None else dict(cp)
            if cp is not None:   # the headline of the block: nothing unexplained on any golden, in either mode
                # (yolov5l6: no 16-bit tolerance is stated -- the reference's own fp16 run pairs 6 of the golden's 27 detections -- so only its fp32 mode counts here; bf16 on the
                #  spread workload likewise: its own bf16 run pairs 23 of 94.  On the LINEAR-REGIME golden both modes count for every architecture)
                modes = lambda k: ("fp32_parity_mode",) if (k != "lin" and (args.arch.endswith("l6_r60") or (k == "spread" and args.dtype == "bf16"))) else ("fp32_parity_mode", f"production_{args.dtype}")  # noqa: E731
                out["parity"]["unexplained"] = sum(cp[k][m_]["unexplained"] for k in ("cond", "spread", "spread_more", "lin") if k in cp for m_ in modes("spread" if k == "spread_more" else k))
                out["parity"]["unexplained_scope"] = ("fp32 mode on every golden + the 16-bit path wherever `stated_tolerance` is not null (cond / spread / lin); blocks with a null "
                                                      "tolerance (yolov5l6 cond, bf16 spread) sit in the regime where the reference's own 16-bit run re-decides most detections "
                                                      "(reference_own_*) and are compared with that run instead (tests/test_golden_gpu.py)")
                out["parity"]["north_star_tolerance"] = ("boxes within 1e-3 IoU: met by the fp32 mode on every golden, at fp32_parity_mode_images_per_s (>= 4000 on C2); the production 16-bit "
                                                         "path is held to stated constant tolerances (cond / spread / lin) and reported against the reference's OWN 16-bit run (reference_own_*): "
                                                         "a per-layer budget (profiles/r04_error_budget_*.csv) shows no 16-bit-storage path can meet 1e-3")
                fp32_checks = {}
                out["parity"]["fp32_parity_mode_images_per_s"] = fp32_mode_throughput(args, dev, images_cpu, checks=fp32_checks)
                if fp32_checks:
                    out["parity"]["fp32_parity_mode_on_benchmark_workload"] = fp32_checks
            out["parity"]["benchmark_workload"] = parity_sample(args, model, images_gpu, images_cpu, sd_cpu, min(k_par, args.batch))
            out["cpu_baseline"] = cpu_baseline(args, sd_cpu, images_cpu)
        if args.per_op and world == 1:
            # the per-op profile replays the recorded plan from its NHWC4 input buffer: fill it through the letterbox
            # path first (identity-size batches normally feed the stem from the planar images and never touch it)
            yolo.stem_from_planar = False
            collect(model.forward_async(images_gpu))
            torch.cuda.synchronize()
            e = next(iter(yolo._entries.values()))
            prof = e.plan.profile(iters=5)
            with open(args.per_op, "w") as f:
                json.dump([{"name": n, "ms": ms, **meta} for n, ms, meta in prof], f, indent=1)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
