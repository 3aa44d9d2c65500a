"""What the workgroup-per-segment NMS kernel (postprocess.hip nms_block_kernel: ymi_nms, YMI_POST_AGNOSTIC) costs or buys against the one-wave kernel.  A record, not a gate.

    python tools/nms_bench.py                    both parts below
    python tools/nms_bench.py --part ops         ymi_nms against ymi_batched_nms with zero labels at n = 64, 1024, 4096, 16384 on rand_boxes and grid_boxes
                                                 (tests/_post_cases.py): device events around `reps` back-to-back calls on preallocated buffers, after a warm-up, reps
                                                 chosen for about a second a row.  On a tree without ymi_nms (the parent commit: --root PATH) only the batched_nms column
                                                 is printed -- that column, taken alternately with this build's in one GPU call, is the yardstick.
    python tools/nms_bench.py --part post        the whole post-process with agnostic=True on 32 images of the 640 x 640 head shapes at nc = 80, both candidate modes,
                                                 in THIS process (YOLORT_AMD_NMS_BLOCK is read once per process); without --part the tool runs it in two child processes,
                                                 YOLORT_AMD_NMS_BLOCK=1 and 0
Every part prints JSON lines."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _events_ms(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _time_row(torch, fn, target_s=1.0):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    once = _events_ms(torch, fn, 10)
    reps = max(10, min(20000, int(target_s * 1000.0 / max(once, 1e-3))))
    return round(_events_ms(torch, fn, reps) * 1000.0, 2), reps   # microseconds per call


def part_ops(root):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import _post_cases as P
    from yolort_amd import _lib
    lib = _lib.load(require_gpu=True)
    dev = torch.device("cuda:0")
    has_nms = hasattr(lib, "ymi_nms") and "ymi_nms" in _lib.EXPORTED_SYMBOLS
    for kind in ("rand_boxes", "grid_boxes"):
        for n in (64, 1024, 4096, 16384):
            rng = np.random.default_rng(n)
            if kind == "rand_boxes":
                boxes = P.rand_boxes(rng, n)
            else:
                side = int(np.ceil(np.sqrt(n / 3.0)))
                boxes = P.grid_boxes(side)[rng.permutation(3 * side * side)[:n]]
            b = torch.from_numpy(np.ascontiguousarray(boxes)).to(dev)
            s = torch.from_numpy(rng.random(n, dtype=np.float32)).to(dev)
            zeros = torch.zeros(n, dtype=torch.int32, device=dev)
            keep, count = torch.empty(n, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            ws = torch.empty(lib.ymi_nms_ws_bytes(n), dtype=torch.uint8, device=dev)
            st = _lib.stream_ptr()

            def batched():
                _lib.check(lib.ymi_batched_nms(b.data_ptr(), s.data_ptr(), zeros.data_ptr(), n, 0.45, keep.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), st))

            def block():
                _lib.check(lib.ymi_nms(b.data_ptr(), s.data_ptr(), n, 0.45, keep.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), st))

            row = {"part": "ops", "root": root, "boxes": kind, "n": n}
            row["batched_nms_us"], row["batched_nms_reps"] = _time_row(torch, batched)
            row["kept"] = int(count.item())
            if has_nms:
                want = keep[: row["kept"]].clone()
                row["nms_us"], row["nms_reps"] = _time_row(torch, block)
                assert int(count.item()) == row["kept"] and torch.equal(keep[: row["kept"]], want), "ymi_nms and ymi_batched_nms disagree"
            print(json.dumps(row), flush=True)


def part_post(root):
    import torch
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import _post_cases as P
    from oracle import yolov5_oracle as O
    from yolort_amd import _lib
    from yolort_amd.engine import Plan, View
    dev = torch.device("cuda:0")
    n, nc, kk, thr, k = 32, 80, 85, 0.25, 300
    shapes = [(80, 80), (40, 40), (20, 20)]
    strides, anchors = O.anchors_for(3)
    heads = P.post_heads(nc, shapes, n=n)
    inputs = []
    for ho in heads:
        ho[..., 4] -= 2.0   # a crowded but not saturated batch
        t = torch.zeros(n, ho.shape[2], ho.shape[3], (3 * kk + 3) // 4 * 4, device=dev, dtype=torch.float32)
        t[..., : 3 * kk] = ho.to(dev).permute(0, 2, 3, 1, 4).reshape(n, ho.shape[2], ho.shape[3], 3 * kk)
        inputs.append(t)
    for mode, base in (("multi_label", 0), ("best_class", _lib.POST_BEST_CLASS)):
        flags, cap = base | _lib.POST_AGNOSTIC, n * 16384
        while True:   # the host protocol of ops.postprocess_logits, once; the plan that came through is the one that is timed
            plan = Plan(dev, torch.float16)
            views = [View(t.view(-1), 0, n, t.shape[1], t.shape[2], 3 * kk, t.shape[3]) for t in inputs]
            pb = plan.postprocess(views, strides, anchors, nc, thr, 0.45, k, cap, flags=flags)
            plan.run()
            st = pb.status.cpu().tolist()
            if st[1] == 0:
                break
            if not st[1] & 1:
                flags |= _lib.POST_EXACT_FULL
                continue
            cap = max(int(max(st[0], st[3] * n) * 1.25) + 1024, 2 * cap)
            cap = n * (1 << ((cap + n - 1) // n - 1).bit_length())
        us, reps = _time_row(torch, plan.run)
        print(json.dumps({"part": "post", "root": root, "NMS_BLOCK": os.environ.get("YOLORT_AMD_NMS_BLOCK", "1"), "mode": mode, "exact_full": bool(flags & _lib.POST_EXACT_FULL),
                          "raw_candidates": st[4], "records_sorted": st[0], "detections": int(pb.count.sum().item()), "post_us": us, "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("ops", "post"), default=None)
    ap.add_argument("--root", default=HERE, help="the tree whose yolort_amd package is measured (default: this one)")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    if args.part == "ops":
        return part_ops(root)
    if args.part == "post":
        return part_post(root)
    part_ops(root)
    for block in ("1", "0"):
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "post", "--root", root], env=dict(os.environ, YOLORT_AMD_NMS_BLOCK=block), capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            raise SystemExit(f"the post part failed with YOLORT_AMD_NMS_BLOCK={block} after {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
