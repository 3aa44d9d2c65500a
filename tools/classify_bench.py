"""What the tail of a second-stage classifier costs on one MI355X: ops.classify_head (pool_fc_kernel, both launches: pooled maps -> Hardswish hidden -> logits) and
ops.second_stage_filter, each against the status quo on the SAME device and inputs, alternating -- the same tail in torch: map.float().mean((1, 2)), F.linear,
F.hardswish, F.linear; argmax and a boolean index.  Shapes: the heads of darknet_s_r6_0 (512 channels) and darknet_l_r6_0 (1024), 1000 classes, 7 x 7 maps, fp16,
n = 8, 256 and 8116 crops (the count the crop and render benches use).  Records the n_split the launcher's rule chose and, at n = 8, one run with n_split forced to 1.
A record, not a gate: no ratio is fixed in advance.

    python tools/classify_bench.py [--out profiles/classify_bench.txt] [--iters 50] [--rounds 5]
Every figure is the median over `rounds` of (device-event time around `iters` back-to-back calls) / iters, the two sides alternating round by round."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify_bench.txt"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F

    from yolort_amd import ops

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = [f"classify_bench on {torch.cuda.get_device_name(0)} ({cus} CUs), torch {torch.__version__}; fp16, 7 x 7 maps, 1000 classes; "
             f"median of {args.rounds} rounds of {args.iters} back-to-back calls, us per call (min .. max of the rounds)"]

    def span(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    def alternating(fns):
        for fn in fns:   # every shape warmed
            fn(); fn()
        torch.cuda.synchronize()
        t = [[] for _ in fns]
        for _ in range(args.rounds):
            for i, fn in enumerate(fns):
                t[i].append(span(fn))
        return [f"{statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})" for v in t], [statistics.median(v) for v in t]

    def rule(nblk, nslices):   # the launcher's rule (csrc/classify_head.hip choose_n_split), restated for the record
        return max(1, min(cus // nblk, nslices))

    g = torch.Generator().manual_seed(0)
    for name, c in (("darknet_s_r6_0", 512), ("darknet_l_r6_0", 1024)):
        w1, b1 = (torch.rand(c, c, generator=g) - 0.5).mul(0.1).to(dev), torch.rand(c, generator=g).to(dev)
        w2, b2 = (torch.rand(1000, c, generator=g) - 0.5).mul(0.1).to(dev), torch.rand(1000, generator=g).to(dev)
        p1, p2 = ops.pack_linear(w1, b1, torch.float16), ops.pack_linear(w2, b2, torch.float16)
        w1h, w2h, b1h, b2h = w1.half(), w2.half(), b1.half(), b2.half()
        for n in (8, 256, 8116):
            fmap = torch.rand(n, 7, 7, c, generator=g).half().to(dev)
            out, hid = torch.empty(n, 1000, device=dev), torch.empty(n, c, device=dev, dtype=torch.float16)
            hip = lambda s=0: ops.classify_head(fmap, p1, None, p2, dtype=torch.float16, n_split=s, out=out, hidden=hid)
            ref = lambda: F.linear(F.hardswish(F.linear(fmap.float().mean((1, 2)).half(), w1h, b1h)), w2h, b2h).float()
            diff = (hip() - ref()).abs().max().item()
            fns = [hip, ref] + ([lambda: hip(1)] if n == 8 else [])
            txt, med = alternating(fns)
            nblk = (n + 31) // 32
            lines.append(f"{name} head n={n:5d}: hip {txt[0]}  torch {txt[1]}  torch/hip {med[1] / med[0]:.2f}  n_split rule {rule(nblk, c // 32)} / {rule(nblk, 32)}"
                         f"  max |hip - torch| {diff:.3e}" + (f"  hip with n_split=1 {txt[2]}" if n == 8 else ""))
    # the filter: 32 images, the crops spread evenly over them
    for n in (8, 256, 8116):
        k = (n + 31) // 32
        counts = torch.tensor([min(k, max(0, n - i * k)) for i in range(32)], dtype=torch.int32, device=dev)
        boxes, scores = torch.rand(32, k, 4, generator=g).to(dev), torch.rand(32, k, generator=g).to(dev)
        logits = torch.randn(n, 1000, generator=g).to(dev)
        labels = torch.zeros(32 * k, dtype=torch.int64)
        valid = (torch.arange(k)[None, :] < counts.cpu()[:, None]).flatten()
        labels[valid] = torch.where(torch.arange(n) % 2 == 0, logits.argmax(1).cpu(), torch.zeros(n, dtype=torch.int64))
        labels = labels.view(32, k).to(dev)
        total = torch.tensor([n, 0], dtype=torch.int32, device=dev)
        flat_b, flat_s, flat_l, valid = boxes.view(-1, 4)[valid.to(dev)], scores.flatten()[valid.to(dev)], labels.flatten()[valid.to(dev)], None

        def ref():   # (the boolean index synchronises: the status quo's own cost)
            keep = logits.argmax(1) == flat_l
            return flat_b[keep], flat_s[keep], flat_l[keep]

        hip = lambda: ops.second_stage_filter(boxes, scores, labels, counts, logits, total)
        assert int(hip()[3].sum()) == ref()[0].shape[0]
        txt, med = alternating([hip, ref])
        lines.append(f"filter n={n:5d} (32 images, K={k}): hip {txt[0]}  torch {txt[1]}  torch/hip {med[1] / med[0]:.2f}  (hip includes the op's six torch.empty calls)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
