"""The attention kernel alone (ymi_attention through Plan.attention, csrc/attention.hip) against the composition a user has today, F.scaled_dot_product_attention on
the same fp16 operands.  Device events around chains of launches over DISTINCT qkv buffers (about 600 MB: more than the 256 MB MALL holds); the two contenders alternate
inside every round, medians are reported with their spread.  Roofline of a launch: flops = 4 n heads S^2 d against the dense fp16 MFMA peak, bytes = q, k, v, o once
against the HBM peak (the peaks bench.py uses); the larger of the two times is the bound.
usage: python tools/attention_bench.py [rounds] [reps]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from yolort_amd import engine

HBM_PEAK, MFMA_PEAK = 8.0e12, 2.5e15
SHAPES = [(32, 20, 20, 256, 4), (32, 40, 40, 128, 4), (8, 40, 40, 512, 4)]   # n, h, w, c, heads
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda:0")


def timed(fn):
    """ms per call of fn() over `reps` calls, device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for n, h, w, c, heads in SHAPES:
    s, d = h * w, c // heads
    flops, nbytes = 4.0 * n * heads * s * s * d, 2 * 4 * n * s * c
    nb = max(4, -(-600_000_000 // nbytes))   # launches per chain
    plan = engine.Plan(dev, torch.float16)
    qkv = [plan.alloc(n, h, w, 3 * c) for _ in range(nb)]
    for v in qkv:
        v.base.normal_()
    outs = [plan.attention(v.slice_c(0, c), v.slice_c(c, c), v.slice_c(2 * c, c), heads) for v in qkv]
    # torch: (n, heads, S, d) views of the same memory, no copy
    tq = [[v.slice_c(i * c, c).as_tensor().reshape(n, s, heads, d).transpose(1, 2) for i in range(3)] for v in qkv]

    def run_torch():
        for q, k, v in tq:
            F.scaled_dot_product_attention(q, k, v)

    plan.run()   # same inputs, same result (fp16 operands, fp32 soft-max on both sides)
    want = F.scaled_dot_product_attention(*(t.float() for t in tq[0])).transpose(1, 2).reshape(n, h, w, c)
    err = float((outs[0].as_tensor().float() - want).abs().max())
    assert err < 4e-3 * max(1.0, float(want.abs().max())), err
    for fn in (plan.run, run_torch):
        fn()
    torch.cuda.synchronize()
    t = {"hip": [], "torch": []}
    for _ in range(rounds):
        t["hip"].append(timed(plan.run) / nb)
        t["torch"].append(timed(run_torch) / nb)
    med = {key: statistics.median(v) for key, v in t.items()}
    t_mfma, t_hbm = flops / MFMA_PEAK * 1e3, nbytes / HBM_PEAK * 1e3
    print(f"attention {n}x{h}x{w}x{c} heads {heads} (d {d}, S {s}) fp16, {nb} launches per chain, {rounds} rounds x {reps} reps, max abs err vs torch fp32 {err:.1e}")
    for key in t:
        print(f"  {key:6s} median {med[key] * 1e3:8.1f} us per launch   (min {min(t[key]) * 1e3:.1f}, max {max(t[key]) * 1e3:.1f})")
    print(f"  hip: {flops / 1e9:.2f} GFLOP -> {flops / med['hip'] / 1e9:.1f} TFLOP/s = {t_mfma / med['hip']:.3f} of the MFMA bound ({t_mfma * 1e3:.1f} us); {nbytes / 1e6:.1f} MB -> "
          f"{nbytes / med['hip'] / 1e9:.2f} TB/s = {t_hbm / med['hip']:.3f} of the HBM bound ({t_hbm * 1e3:.1f} us); {med['torch'] / med['hip']:.2f}x F.scaled_dot_product_attention")
