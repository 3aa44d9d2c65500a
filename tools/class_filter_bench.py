"""What the class filter (classes=[...], YMI_POST_CLASS_FILTER) costs or buys end to end: the C2 workload of bench.py (yolov5s fp16, 32 x 640 x 640, score_thresh 0.25, the
seeded weights of workloads/synth.py at head_gain 0.4) run through the serving loop with classes=None, classes=[0] and a 9-class set, in both candidate modes, alternating,
with the raw candidate count (status[4]: what the producers wrote AFTER the filter) and the records sorted (status[0]) of each.  A record, not a gate: bench.py cannot select
the filter.

    python tools/class_filter_bench.py [--steps 60] [--warmup 10] [--repeats 5] [--batch 32] [--size 640]
prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = {"none": None, "one": (0,), "nine": (0, 2, 5, 7, 27, 31, 58, 64, 79)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--arch", default="yolov5_darknet_pan_s_r60")
    ap.add_argument("--score-thresh", type=float, default=0.25)
    ap.add_argument("--head-gain", type=float, default=0.4)
    args = ap.parse_args()

    import torch

    from workloads.synth import synth_images, synth_weights
    from yolort_amd.models import YOLOv5

    dev = torch.device("cuda:0")
    images = [im.to(dev).half() for im in synth_images(args.batch, args.size, args.size, seed=1)]
    models = {}
    for mode, multi in (("multi_label", True), ("best_class", False)):
        for name, classes in SETS.items():
            m = YOLOv5(arch=args.arch, size=(args.size, args.size), score_thresh=args.score_thresh, nms_thresh=0.45, detections_per_img=300, multi_label=multi, classes=classes)
            m.load_state_dict(synth_weights(m.state_dict(), args.arch, seed=0, head_gain=args.head_gain))
            models[f"{mode}/{name}"] = m.to(dev).half().eval()

    def run_steps(m, k):
        depth = max(1, m.model.pipeline_depth - 1)
        pending, dets = [], None
        for _ in range(k):
            pending.append(m.forward_async(images))
            if len(pending) > depth:
                dets = pending.pop(0).result()
        while pending:
            dets = pending.pop(0).result()
        return dets

    out = {}
    for key, m in models.items():
        dets = run_steps(m, max(args.warmup, 1))
        torch.cuda.synchronize()
        e = next(iter(m.model._entries.values()))
        out[key] = {"classes": SETS[key.split("/")[1]], "raw_candidates_status4": int(e.post.status[4].item()), "records_sorted_status0": int(e.post.status[0].item()),
                    "detections": sum(len(d["scores"]) for d in dets), "img_per_s": []}
    for _ in range(args.repeats):   # alternating: every series sees the same clocks
        for key, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(m, args.steps)
            torch.cuda.synchronize()
            out[key]["img_per_s"].append(round(args.steps * args.batch / (time.perf_counter() - t0), 1))
    for key in out:
        out[key]["median_img_per_s"] = statistics.median(out[key]["img_per_s"])
    print(json.dumps({"workload": f"{args.arch} fp16 {args.batch}x{args.size}x{args.size} thr {args.score_thresh} head_gain {args.head_gain}", "steps": args.steps,
                      "device": torch.cuda.get_device_name(0), **out}))


if __name__ == "__main__":
    main()
