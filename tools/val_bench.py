"""What YOLOv5's validation numbers cost on the host and on the device: the NumPy restatement of the matching (tests/_val_cases.py model, a loop over the images with
the two `unique` steps) followed by metrics.val_summary, against metrics.ValEvaluator and metrics.ConfusionMatrix (one val_match_kernel launch per batch each) on the
SAME inputs and the same machine.  The inputs are tools/eval_bench.py's: the detections of bench.py's C2 workload -- one 32-image batch written by
`python bench.py --gpus 1 --dump-outputs DIR` -- against the golden detections of that workload (tests/golden/bench_c2.npz; image i against golden image i % 8).
A record, not a gate: bench.py does not use these evaluators.

    python tools/val_bench.py --dets DIR [--repeats 20] [--host-repeats 5]
prints one JSON line.  The variants alternate inside every repeat (launch in matrix mode, launch in tp mode; host, device), so that a drift of the machine meets all
of them alike."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", required=True, help="directory holding boxes.npy, scores.npy, labels.npy, counts.npy as bench.py --dump-outputs writes them")
    ap.add_argument("--golden", default=os.path.join(ROOT, "tests", "golden", "bench_c2.npz"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--num-classes", type=int, default=80)
    args = ap.parse_args()

    import numpy as np
    import torch

    import _val_cases as V
    from yolort_amd import ops
    from yolort_amd.utils import metrics as M

    dev = torch.device("cuda:0")
    C = args.num_classes
    a = {k: np.load(os.path.join(args.dets, k + ".npy")) for k in ("boxes", "scores", "labels", "counts")}
    n, k = a["scores"].shape
    z = np.load(args.golden)
    n_gold = len(json.loads(str(z["meta"]))["dets"])
    targets = [{"boxes": z[f"det{i % n_gold}_boxes"], "labels": z[f"det{i % n_gold}_labels"]} for i in range(n)]
    slab = (torch.from_numpy(a["boxes"]).to(dev), torch.from_numpy(a["scores"]).to(dev), torch.from_numpy(a["labels"]).to(torch.int64).to(dev),
            torch.from_numpy(a["counts"]).to(torch.int32).to(dev))
    gt = M.GpuDetectionEvaluator._pad_targets(targets, dev)
    case = dict(C=C, boxes=a["boxes"].astype(np.float32), scores=a["scores"].astype(np.float32), labels=a["labels"].astype(np.int64), counts=a["counts"].astype(np.int32),
                gt_boxes=gt[0].cpu().numpy(), gt_labels=gt[1].cpu().numpy(), gt_counts=gt[2].cpu().numpy())
    iouv = [float(t) for t in M.VAL_IOUV]
    matrix = torch.zeros(C + 1, C + 1, device=dev, dtype=torch.int32)
    status = torch.zeros(4, device=dev, dtype=torch.int32)
    variants = {"matrix": dict(conf=0.25, thrs=[0.45], class_aware=False, matrix=matrix, status=status),
                "tp": dict(conf=float("-inf"), thrs=iouv, class_aware=True, status=status)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(3):   # warm-up: module load, allocator
        for kw in variants.values():
            ops.val_match(*slab, *gt, C, **kw)
    torch.cuda.synchronize()
    launch_ms = {name: [] for name in variants}
    update_ms = []
    for _ in range(args.repeats):
        for name, kw in variants.items():
            launch_ms[name].append(timed(lambda: ops.val_match(*slab, *gt, C, **kw)))
        ev = M.ValEvaluator(C)
        update_ms.append(timed(lambda: ev.update_from_slab(slab, gt)))

    # the kernel by itself: 50 launches captured into one graph and replayed, so that the wrapper's Python and the launch gaps are out of the bracket
    kernel_ms = {}
    for name, kw in variants.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(50):
                ops.val_match(*slab, *gt, C, **kw)
        g.replay()
        torch.cuda.synchronize()
        kernel_ms[name] = round(statistics.median(timed(g.replay) for _ in range(args.repeats)) / 50, 5)

    def host_val():
        live = np.arange(k)[None, :] < case["counts"][:, None]
        tp = V.model(case, float("-inf"), iouv, True)[2]
        glive = np.arange(case["gt_labels"].shape[1])[None, :] < case["gt_counts"][:, None]
        return M.val_summary(tp[live], case["scores"][live], case["labels"][live], case["gt_labels"][glive])

    def dev_val():
        ev = M.ValEvaluator(C)
        ev.update_from_slab(slab, gt)
        return ev.compute()

    def host_cm():
        return V.model(case, 0.25, [0.45], False)[3]

    def dev_cm():
        cm = M.ConfusionMatrix(C)
        cm.update_from_slab(slab, gt)
        return cm.matrix

    wall = {"host_val": [], "dev_val": [], "host_cm": [], "dev_cm": []}
    res = {}
    for _ in range(args.host_repeats):
        for name, fn in (("host_val", host_val), ("dev_val", dev_val), ("host_cm", host_cm), ("dev_cm", dev_cm)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[name] = fn()
            wall[name].append(time.perf_counter() - t0)
    med = {name: statistics.median(v) for name, v in wall.items()}
    print(json.dumps({
        "inputs": f"{n} images x {k} slots, {int(a['counts'].sum())} detections, up to {int(case['gt_counts'].max())} ground truths per image, {C} classes",
        "device": torch.cuda.get_device_name(0),
        "val_match_launch_ms_median": {name: round(statistics.median(v), 4) for name, v in launch_ms.items()},
        "val_match_launch_ms_min_max": {name: [round(min(v), 4), round(max(v), 4)] for name, v in launch_ms.items()},
        "val_match_kernel_ms_in_graph_of_50": kernel_ms,
        "val_evaluator_update_from_slab_ms_median": round(statistics.median(update_ms), 4),
        "wall_s_median": {name: round(v, 5) for name, v in med.items()}, "wall_s_all": {name: [round(x, 5) for x in v] for name, v in wall.items()},
        "ratio_host_over_device_val_update_plus_compute": round(med["host_val"] / med["dev_val"], 1),
        "ratio_host_over_device_confusion_matrix": round(med["host_cm"] / med["dev_cm"], 1),
        "val_dicts_equal": res["host_val"] == res["dev_val"], "matrices_equal": bool((res["host_cm"] == res["dev_cm"]).all()),
        "matrix_sum": int(res["dev_cm"].sum()), "val": {k_: v for k_, v in res["dev_val"].items() if not k_.endswith("_class")}}))


if __name__ == "__main__":
    main()
