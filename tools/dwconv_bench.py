"""The depthwise kernel alone (ymi_dwconv2d through Plan.dwconv, csrc/dwconv.hip) against F.conv2d(groups=c) on channels-last fp16 and against the library's plain
16-byte copy kernel on the same byte count -- the floor of a streaming kernel.  Device events around chains of launches over DISTINCT buffers (more than the 256 MB
MALL holds, so nothing is re-read from cache between launches); the three contenders alternate inside every round, rounds are reported with their spread.
Bytes of a launch = input + output (weights are a few KiB): what the algorithm needs, not what the kernel moves.
usage: python tools/dwconv_bench.py [rounds] [reps]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from yolort_amd import engine
from yolort_amd._lib import ACT_SILU

SHAPES = [(32, 80, 80, 64, 5, 1), (32, 40, 40, 128, 3, 2), (32, 20, 20, 256, 5, 1)]   # n, h, w, c, k, s
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


for n, h, w, c, k, s in SHAPES:
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    nbytes = 2 * n * c * (h * w + ho * wo)
    nb = max(4, -(-600_000_000 // nbytes))   # launches per chain: 600 MB of distinct buffers
    torch.manual_seed(0)
    wt = torch.randn(c, 1, k, k) * 0.2
    bias = torch.randn(c) * 0.1
    # ours: a plan of nb depthwise launches (SiLU epilogue, as GhostConv.cv2 runs it)
    plan = engine.Plan(dev, torch.float16)
    pd = engine.PackedDWConv(wt, bias, None, torch.float16, dev)
    xs = [plan.alloc(n, h, w, c) for _ in range(nb)]
    for v in xs:
        v.base.normal_()
    ys = [plan.dwconv(v, pd, k, s, ACT_SILU) for v in xs]
    # the copy floor: the same bytes through copy_view_kernel (a c_copy-channel copy of the input map moves input + output bytes)
    c_copy = c * (h * w + ho * wo) // (2 * h * w) // 8 * 8
    cplan = engine.Plan(dev, torch.float16)
    cs = [cplan.alloc(n, h, w, c_copy) for _ in range(nb)]
    for v in cs:
        v.base.normal_()
    for v in cs:
        cplan.copy(v, cplan.alloc(n, h, w, c_copy))
    copy_bytes = 2 * 2 * n * h * w * c_copy
    # torch: F.conv2d(groups=c) + bias + SiLU on channels-last fp16 (MIOpen's depthwise path, then the activation as torch runs it)
    txs = [v.as_tensor().permute(0, 3, 1, 2) for v in xs]   # NCHW views of the same NHWC memory = channels_last
    tw, tb = wt.to(dev).half().contiguous(memory_format=torch.channels_last), bias.to(dev).half()
    assert txs[0].is_contiguous(memory_format=torch.channels_last)

    def run_torch():
        for t in txs:
            F.silu(F.conv2d(t, tw, tb, s, k // 2, groups=c))

    def run_torch_conv_only():
        for t in txs:
            F.conv2d(t, tw, tb, s, k // 2, groups=c)

    # same seeded inputs, same result (measuring-on-mi355x section 6): fp16 storage, fp32 accumulation on both sides
    plan.run()
    want = F.silu(F.conv2d(txs[0].float(), wt.to(dev), bias.to(dev), s, k // 2, groups=c)).permute(0, 2, 3, 1)
    err = float((ys[0].as_tensor().float() - want).abs().max()) / max(1.0, float(want.abs().max()))
    assert err < 2e-3, err
    for fn in (plan.run, cplan.run, run_torch, run_torch_conv_only):   # warm-up of everything the timed windows use
        fn()
    torch.cuda.synchronize()
    t = {"hip": [], "copy": [], "torch": [], "torch_conv": []}
    for _ in range(rounds):
        t["hip"].append(timed(plan.run) / nb)
        t["torch"].append(timed(run_torch) / nb)
        t["copy"].append(timed(cplan.run) / nb)
        t["torch_conv"].append(timed(run_torch_conv_only) / nb)
    med = {key: statistics.median(v) for key, v in t.items()}
    rate = nbytes / med["hip"] / 1e9
    copy_rate = copy_bytes / med["copy"] / 1e9
    print(f"dwconv {n}x{h}x{w}x{c} k{k} s{s} fp16, {nb} launches per chain, {rounds} rounds x {reps} reps, max rel err vs torch fp32 {err:.1e}")
    for key in t:
        print(f"  {key:10s} median {med[key] * 1e3:8.1f} us per launch   (min {min(t[key]) * 1e3:.1f}, max {max(t[key]) * 1e3:.1f})")
    print(f"  hip: {nbytes / 1e6:.1f} MB algorithmic -> {rate:.2f} TB/s = {rate / copy_rate:.2f} of the copy kernel's {copy_rate:.2f} TB/s on {copy_bytes / 1e6:.1f} MB; "
          f"{med['torch'] / med['hip']:.2f}x F.conv2d(groups=c) + SiLU, {med['torch_conv'] / med['hip']:.2f}x the convolution alone")
