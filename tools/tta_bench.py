"""What augmented inference (augment=True: test-time augmentation, ultralytics' _forward_augment) costs end to end: the C2 workload of bench.py (yolov5s fp16, 32 x 640 x 640,
the seeded weights of workloads/synth.py at head_gain 0.4) run through the serving loop with `augment` off and on, alternating.  The durations of the two new kernels
(scale_view_kernel: two launches per batch, 544 x 544 mirrored and 448 x 448; decode_view_kernel: seven launches per batch, the kept levels of the three views) and of the
kernel the view decode is the twin of come from torch.profiler's kernel records of a few serial steps of each model (null when the profiler sees no kernels).  A record, not a
gate: bench.py cannot select the option.

    python tools/tta_bench.py [--steps 60] [--warmup 10] [--repeats 5] [--batch 32] [--size 640] [--score-thresh 0.25]
prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"off": dict(augment=False), "augment": dict(augment=True)}
KERNELS = ("scale_view_kernel", "decode_view_kernel", "decode_kernel")


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

    def make(**kw):
        m = YOLOv5(arch=args.arch, size=(args.size, args.size), score_thresh=args.score_thresh, nms_thresh=0.45, detections_per_img=300, **kw)
        m.load_state_dict(synth_weights(m.state_dict(), args.arch, seed=0, head_gain=args.head_gain))
        return m.to(dev).half().eval()

    models = {name: make(**kw) for name, kw in MODES.items()}

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

    def kernel_us(m):
        """total duration per step of each kernel of KERNELS (all its launches of a batch), and the launches per step, over a few serial steps"""
        try:
            from torch.profiler import ProfilerActivity, profile
            steps = 5
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(steps):
                    m(images)
                torch.cuda.synchronize()
            out = {}
            for ev in prof.key_averages():
                for name in KERNELS:
                    if name in ev.key and not (name == "decode_kernel" and "view" in ev.key):
                        total = float(getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0))
                        cur = out.setdefault(name, {"us_per_step": 0.0, "launches_per_step": 0.0})
                        cur["us_per_step"] = round(cur["us_per_step"] + total / steps, 2)
                        cur["launches_per_step"] = round(cur["launches_per_step"] + ev.count / steps, 2)
            return out or None
        except Exception as e:  # noqa: BLE001
            return {"error": str(e)[:200]}

    out = {}
    for key, m in models.items():
        dets = run_steps(m, max(args.warmup, 1))
        torch.cuda.synchronize()
        e = next(iter(m.model._entries.values()))
        out[key] = {"plan_ops": e.plan.num_ops, "raw_candidates_status4": int(e.post.status[4].item()), "detections": sum(len(d["scores"]) for d in dets),
                    "cand_cap_per_image": m.model.cand_cap_per_image, "img_per_s": []}
    for _ in range(args.repeats):   # alternating: every series sees the same clocks
        for key, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(m, args.steps)
            torch.cuda.synchronize()
            out[key]["img_per_s"].append(round(args.steps * args.batch / (time.perf_counter() - t0), 1))
    for key, m in models.items():
        out[key]["median_img_per_s"] = statistics.median(out[key]["img_per_s"])
        out[key]["kernel_us"] = kernel_us(m)
    out["augment_over_off"] = round(out["augment"]["median_img_per_s"] / out["off"]["median_img_per_s"], 4)
    print(json.dumps({"workload": f"{args.arch} fp16 {args.batch}x{args.size}x{args.size} thr {args.score_thresh} head_gain {args.head_gain}", "steps": args.steps,
                      "device": torch.cuda.get_device_name(0), **out}))


if __name__ == "__main__":
    main()
