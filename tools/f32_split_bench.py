"""Per-launch A/B of the fp32 mode's convolutions: the exact fp32 tiles 20x against their split-bf16 forms 21x (6 products) and 22x (8 products), csrc/conv_f32_split.hip.

    python tools/f32_split_bench.py [--config c2] [--reps 7] > profiles/f32_split_bench.txt

Three plans of the same network and batch (YOLORT_AMD_F32_SPLIT unset / 6 / 8), each on its own buffers, are profiled in turn (`Plan.profile`: device events around every
launch of the recorded plan), `--reps` rounds with the contenders alternating; the table holds the MEDIAN per launch and the three stack totals.  Not a test: it needs an
MI355X and prints what it measured.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


def build(config, batch, split):
    from yolort_amd.models import YOLOv5
    from workloads.synth import synth_images, synth_weights
    c = bench.CONFIGS[config]
    if split:
        os.environ["YOLORT_AMD_F32_SPLIT"] = split
    else:
        os.environ.pop("YOLORT_AMD_F32_SPLIT", None)
    dev = torch.device("cuda:0")
    m = YOLOv5(arch=c["arch"], size=(c["size"], c["size"]), score_thresh=c["score_thresh"], nms_thresh=0.45, detections_per_img=300)
    m.load_state_dict(synth_weights(m.state_dict(), c["arch"], seed=0, head_gain=c["head_gain"]))
    m = m.to(dev).eval().set_compute_dtype(torch.float32)
    m.model.pipeline_depth = 1
    imgs = [im.to(dev) for im in synth_images(batch, c["size"], c["size"], seed=1)]
    for _ in range(2):   # the plan is built (and the switch read) by the first forward
        m.forward(imgs)
    torch.cuda.synchronize()
    return m, next(iter(m.model._entries.values())).plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    names = ["20x", "21x", "22x"]
    built = [build(a.config, a.batch, s) for s in ("", "6", "8")]   # (the models keep their plans alive)
    plans = [p for _, p in built]
    os.environ.pop("YOLORT_AMD_F32_SPLIT", None)
    runs = [[] for _ in plans]
    for _ in range(a.reps):
        for i, p in enumerate(plans):   # contenders alternate within a round
            runs[i].append(p.profile(iters=3))
    nops = len(runs[0][0])
    assert all(len(r) == nops for rr in runs for r in rr), "the three plans hold the same launches"
    print(f"# {a.config} batch {a.batch} fp32 mode, median of {a.reps} rounds x 3 timed launches, us; ratio = 20x time / split time")
    print("op,name,shape,tile_20x,us_20x,tile_21x,us_21x,ratio_21x,tile_22x,us_22x,ratio_22x")
    tot = [0.0, 0.0, 0.0]
    slower = []
    for op in range(nops):
        name, _, meta = runs[0][0][op]
        if meta.get("kind") != "conv":
            continue
        us = [statistics.median(r[op][1] for r in runs[i]) * 1e3 for i in range(3)]
        tiles = [runs[i][0][op][2].get("tile") for i in range(3)]
        for i in range(3):
            tot[i] += us[i]
        if min(us[1], us[2]) > us[0]:
            slower.append(name)
        print(f"{op},{name},{meta.get('shape', '')},{tiles[0]},{us[0]:.1f},{tiles[1]},{us[1]:.1f},{us[0] / us[1]:.2f},{tiles[2]},{us[2]:.1f},{us[0] / us[2]:.2f}")
    print("# conv stack per step: " + ", ".join(f"{n} {t:.0f} us" for n, t in zip(names, tot)) + f"; 20x / 21x = {tot[0] / tot[1]:.2f}, 20x / 22x = {tot[0] / tot[2]:.2f}")
    print(f"# launches where both split forms are slower than the 20x tile: {slower or 'none'}")


if __name__ == "__main__":
    main()
