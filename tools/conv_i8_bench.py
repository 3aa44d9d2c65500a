"""The int8 convolution (ymi_conv2d_i8 through Plan.conv_i8, int8 in and out, csrc/conv_i8.hip) against the project's own fp16 convolution (Plan.conv, whatever tile
the plan picks) on the same shapes, SiLU epilogue on both.  Device events around chains of launches over DISTINCT buffers (more than the 256 MB MALL holds); the two
contenders alternate inside every round; medians and spread are reported.  Each side is put against ITS OWN bounds: algorithmic bytes (input + output + weights) over
the HBM peak, and 2 n ho wo cout cin k^2 operations over the dense matrix peak of its data type.
usage: python tools/conv_i8_bench.py [rounds] [reps]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from yolort_amd import engine
from yolort_amd._lib import ACT_SILU

HBM_TBS, F16_TFLOPS, I8_TOPS = 8.0, 2516.0, 5033.0   # MI355X peaks: HBM3E bandwidth, dense fp16 and int8 matrix rates (AMD's published figures)
SHAPES = [(32, 80, 80, 64, 64, 3, 1), (32, 40, 40, 128, 256, 3, 2), (32, 20, 20, 512, 512, 1, 1)]   # n, h, w, cin, cout, k, s
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
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


for n, h, w, cin, cout, k, s in SHAPES:
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    ops = 2.0 * n * ho * wo * cout * cin * k * k
    elems_in, elems_out, elems_w = n * h * w * cin, n * ho * wo * cout, cout * cin * k * k
    nb = max(4, -(-600_000_000 // (2 * (elems_in + elems_out))))   # launches per chain: 600 MB of distinct fp16 buffers (300 MB of int8 ones)
    torch.manual_seed(0)
    wt, bias = torch.randn(cout, cin, k, k) * (2.0 / (cin * k * k)) ** 0.5, torch.randn(cout) * 0.1
    in_scale, out_scale = 4.0 / 127, 4.0 / 127
    pf = engine.PackedConv(wt, bias, None, torch.float16, dev)
    pq = engine.PackedConvI8(wt, bias, None, in_scale, dev)
    fplan, qplan = engine.Plan(dev, torch.float16), engine.Plan(dev, torch.float16)
    fx = [fplan.alloc(n, h, w, cin) for _ in range(nb)]
    qx = [qplan.alloc(n, h, w, cin, torch.int8) for _ in range(nb)]
    for f, q in zip(fx, qx):
        f.as_tensor().normal_()   # (the view only: the buffer's zero tail stays zero)
        q.as_tensor().copy_(torch.clamp(torch.round(f.as_tensor().float() / in_scale), -127, 127))
    fy = [fplan.conv(v, pf, s, k // 2, ACT_SILU) for v in fx]
    qy = [qplan.conv_i8(v, pq, s, ACT_SILU, out_scale=out_scale) for v in qx]
    # same seeded inputs, comparable results (measuring-on-mi355x section 6): the int8 result against the fp16 one, in units of the output step
    fplan.run()
    qplan.run()
    torch.cuda.synchronize()
    step_err = float((qy[0].as_tensor().float() * out_scale - fy[0].as_tensor().float().clamp(-4, 4)).abs().max()) / out_scale
    for fn in (fplan.run, qplan.run):
        fn()
    torch.cuda.synchronize()
    t = {"fp16": [], "int8": []}
    for _ in range(rounds):
        t["fp16"].append(timed(fplan.run) / nb)
        t["int8"].append(timed(qplan.run) / nb)
    med = {key: statistics.median(v) for key, v in t.items()}
    bytes_of = {"fp16": 2.0 * (elems_in + elems_out + elems_w), "int8": 1.0 * (elems_in + elems_out + elems_w)}
    peak = {"fp16": F16_TFLOPS, "int8": I8_TOPS}
    print(f"conv {n}x{h}x{w} {cin}->{cout} k{k} s{s} SiLU, {nb} launches per chain, {rounds} rounds x {reps} reps; int8 vs fp16 result: max {step_err:.2f} output steps apart")
    for key in t:
        us = med[key] * 1e3
        hbm_us, mfma_us = bytes_of[key] / (HBM_TBS * 1e12) * 1e6, ops / (peak[key] * 1e12) * 1e6
        bound, which = max(hbm_us, mfma_us), "HBM" if hbm_us >= mfma_us else "MFMA"
        print(f"  {key}  median {us:8.1f} us per launch (min {min(t[key]) * 1e3:.1f}, max {max(t[key]) * 1e3:.1f});  HBM bound {hbm_us:6.1f} us, MFMA bound {mfma_us:6.1f} us"
              f" -> {bound / us:.2f} of its {which} bound;  {ops / us / 1e6:7.1f} T(FL)OP/s, {bytes_of[key] / us / 1e6:6.2f} TB/s")
    print(f"  int8 / fp16 time: {med['int8'] / med['fp16']:.2f}  ({'int8' if med['int8'] < med['fp16'] else 'fp16'} wins)")
