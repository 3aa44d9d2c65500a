"""What scoring a batch costs on the host and on the device: metrics.DetectionEvaluator (the pure-Python matching of coco_ap, six passes) against
metrics.GpuDetectionEvaluator (one eval_match_kernel launch per batch, the float64 accumulation on the host) on the SAME inputs and the same machine.  The inputs are the
detections of bench.py's C2 workload -- one 32-image batch written by `python bench.py --gpus 1 --dump-outputs DIR` -- scored against the reference's detections of
that workload (tests/golden/bench_c2.npz) as ground truth.  The golden holds the first 8 images of the batch: image i is scored against golden image i % 8, so the
images from 8 on meet another image's boxes -- the same amount of matching work, a lower AP.  A record, not a gate: bench.py does not use the device evaluator.

    python tools/eval_bench.py --dets DIR [--repeats 20]
prints one JSON line: the kernel time per batch (device events around the launch alone and around the whole update_from_slab), the wall time of both compute()s and of
the host's update_from_slab, the ratio host / device of update + compute, and whether the two dicts are equal."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", required=True, help="directory holding boxes.npy, scores.npy, labels.npy, counts.npy as bench.py --dump-outputs writes them")
    ap.add_argument("--golden", default=os.path.join(ROOT, "tests", "golden", "bench_c2.npz"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--num-classes", type=int, default=80)
    args = ap.parse_args()

    import numpy as np
    import torch

    from yolort_amd import ops
    from yolort_amd.utils import metrics as M

    dev = torch.device("cuda:0")
    a = {k: np.load(os.path.join(args.dets, k + ".npy")) for k in ("boxes", "scores", "labels", "counts")}
    n, k = a["scores"].shape
    slab_host = (torch.from_numpy(a["boxes"]), torch.from_numpy(a["scores"]), torch.from_numpy(a["labels"]).to(torch.int64), torch.from_numpy(a["counts"]).to(torch.int32))
    slab = tuple(t.to(dev) for t in slab_host)
    z = np.load(args.golden)
    n_gold = len(json.loads(str(z["meta"]))["dets"])
    targets = [{"boxes": z[f"det{i % n_gold}_boxes"], "labels": z[f"det{i % n_gold}_labels"]} for i in range(n)]
    g = max(len(t["labels"]) for t in targets)

    # ---- host ----
    host = M.DetectionEvaluator(args.num_classes)
    t0 = time.perf_counter()
    host.update_from_slab(slab_host, targets)
    t1 = time.perf_counter()
    want = host.compute()
    t2 = time.perf_counter()

    # ---- device ----
    gt = M.GpuDetectionEvaluator._pad_targets(targets, dev)
    thrs = M.eval_threshold_set()[0]
    launch_ms, update_ms = [], []
    for _ in range(3):   # warm-up: module load, allocator
        ops._launch_eval_match(*slab, *gt, args.num_classes, thrs, M.EVAL_AREA_RNGS, M.COCO_MAX_DETS)
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops._launch_eval_match(*slab, *gt, args.num_classes, thrs, M.EVAL_AREA_RNGS, M.COCO_MAX_DETS)
        e1.record()
        torch.cuda.synchronize()
        launch_ms.append(e0.elapsed_time(e1))
    for _ in range(args.repeats):
        ev = M.GpuDetectionEvaluator(args.num_classes)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ev.update_from_slab(slab, gt)
        e1.record()
        torch.cuda.synchronize()
        update_ms.append(e0.elapsed_time(e1))
    compute_s = []
    for _ in range(5):
        ev = M.GpuDetectionEvaluator(args.num_classes)
        ev.update_from_slab(slab, gt)
        torch.cuda.synchronize()
        c0 = time.perf_counter()
        got = ev.compute()
        compute_s.append(time.perf_counter() - c0)
    dev_total = statistics.median(update_ms) / 1e3 + statistics.median(compute_s)
    print(json.dumps({
        "inputs": f"{n} images x {k} slots, {int(a['counts'].sum())} detections, up to {g} ground truths per image, {args.num_classes} classes",
        "device": torch.cuda.get_device_name(0),
        "host_update_from_slab_s": round(t1 - t0, 4), "host_compute_s": round(t2 - t1, 4),
        "eval_match_launch_ms_median": round(statistics.median(launch_ms), 4), "eval_match_launch_ms_min_max": [round(min(launch_ms), 4), round(max(launch_ms), 4)],
        "gpu_update_from_slab_ms_median": round(statistics.median(update_ms), 4),
        "gpu_compute_s_median": round(statistics.median(compute_s), 4), "gpu_compute_s_all": [round(c, 4) for c in compute_s],
        "ratio_host_over_device_update_plus_compute": round((t2 - t0) / dev_total, 1),
        "dicts_equal": got == want, "host": want, "gpu": got}))


if __name__ == "__main__":
    main()
