"""What NV12 ingest costs: 32 frames of 1080 x 1920 letterboxed onto the model's 640 canvas in fp16 by
  tiled      letterbox_nv12_tile_kernel (YCbCr -> RGB fused into the staging), per rows-per-wave value
  pixel      letterbox_nv12_kernel (YOLORT_AMD_LETTERBOX=pixel: four taps converted on the fly)
  floor      ymi_letterbox(YMI_U8_HWC) on the PRE-CONVERTED RGB8 frames: twice the source bytes, no conversion
  status quo the torch composition on the same inputs -- chroma repeat_interleave, matrix multiply, clamp, uint8 cast -- followed by ymi_letterbox
alternating, device events around each call; then forward_nv12 against forward on pre-converted frames on bench.py's C2-shaped batch.  A record, not a gate.

    python tools/nv12_bench.py [--repeats 30] [--frames 32]
prints one JSON line per measurement: median and spread of the time per batch, bytes moved (source bytes the path must read + canvas bytes written) over that time,
and the ratios to the floor and to the status quo."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--hw", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()

    import torch

    from yolort_amd import _lib, ops
    from yolort_amd.models import YOLOv5
    from yolort_amd.models.transform import YOLOTransform

    if not torch.cuda.is_available():
        raise SystemExit("nv12_bench needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda:0")
    n, (h, w) = args.frames, args.hw
    g = torch.Generator().manual_seed(3)
    frames = [torch.randint(0, 256, (h * 3 // 2, w), generator=g, dtype=torch.uint8).to(dev) for _ in range(n)]
    tr = YOLOTransform(640, 640)
    (hb, wb), sizes, pads = tr.geometry([(h, w)] * n)
    rgbs = [ops.nv12_to_rgb(f) for f in frames]
    canvas_bytes = n * hb * wb * 4 * 2
    nv12_bytes, rgb_bytes = n * h * w * 3 // 2, n * h * w * 3
    k = torch.tensor(_lib.NV12_COEF[("bt601", False)], dtype=torch.float32, device=dev) / 16384

    def fused():
        return ops.letterbox_nv12(frames, sizes, pads, (hb, wb))

    def floor():
        return tr(rgbs, dtype=torch.float16)[0].view.base.view(n, hb, wb, 4)

    def status_quo():   # the conversion a user writes in torch today (float, rounded to nearest), then the library's letterbox
        out = []
        for f in frames:
            y = f[:h].float() - 16
            c = f[h:].view(h // 2, w // 2, 2).float().repeat_interleave(2, 0).repeat_interleave(2, 1) - 128
            rgb = torch.stack([k[0] * y + k[1] * c[..., 1], k[0] * y + k[2] * c[..., 0] + k[3] * c[..., 1], k[0] * y + k[4] * c[..., 0]], -1)
            out.append(rgb.round().clamp(0, 255).to(torch.uint8))
        return tr(out, dtype=torch.float16)[0].view.base.view(n, hb, wb, 4)

    def with_env(fn, knob):
        def run():
            old = os.environ.pop("YOLORT_AMD_LETTERBOX", None)
            if knob is not None:
                os.environ["YOLORT_AMD_LETTERBOX"] = knob
            try:
                return fn()
            finally:
                os.environ.pop("YOLORT_AMD_LETTERBOX", None)
                if old is not None:
                    os.environ["YOLORT_AMD_LETTERBOX"] = old
        return run

    paths = {"tiled-default": (with_env(fused, None), nv12_bytes), "tiled-rpw1": (with_env(fused, "1"), nv12_bytes), "tiled-rpw2": (with_env(fused, "2"), nv12_bytes),
             "pixel": (with_env(fused, "pixel"), nv12_bytes), "floor-rgb8": (floor, rgb_bytes), "status-quo-torch": (status_quo, nv12_bytes)}
    ref = floor()
    for name, (fn, _) in paths.items():   # warm-up, and the results must not differ: the status quo rounds in float (a few codes may differ), the others are bit-identical
        out = fn()
        torch.cuda.synchronize()
        if name != "status-quo-torch":
            assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), name
    ms = {name: [] for name in paths}
    for _ in range(args.repeats):   # alternating
        for name, (fn, _) in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name, (_, src) in paths.items():
        print(json.dumps({"path": name, "frames": n, "hw": [h, w], "canvas": [hb, wb], "ms_median": round(med[name], 4), "ms_min": round(min(ms[name]), 4),
                          "ms_max": round(max(ms[name]), 4), "GB_per_s": round((src + canvas_bytes) / med[name] / 1e6, 1), "vs_floor": round(med[name] / med["floor-rgb8"], 3),
                          "vs_status_quo": round(med[name] / med["status-quo-torch"], 3)}))
    if args.skip_model:
        return

    # forward_nv12 against forward on pre-converted frames: bench.py's C2 shape (32 images of 576 x 736 -> 512 x 640), yolov5s fp16, seeded weights
    from workloads.synth import synth_weights
    arch = "yolov5_darknet_pan_s_r60"
    m = YOLOv5(arch=arch, size=(640, 640), score_thresh=0.25)
    m.load_state_dict(synth_weights(m.state_dict(), arch, seed=0, head_gain=1.0))
    m = m.to(dev).half().eval()
    fr = [torch.randint(0, 256, (576 * 3 // 2, 736), generator=g, dtype=torch.uint8).to(dev) for _ in range(32)]
    pre = [ops.nv12_to_rgb(f) for f in fr]
    runs = {"forward_nv12": lambda: m.forward_nv12(fr), "forward-rgb8": lambda: m(pre)}
    tms = {name: [] for name in runs}
    for name, fn in runs.items():
        for _ in range(3):
            fn()
    for _ in range(args.repeats):
        for name, fn in runs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            tms[name].append(e0.elapsed_time(e1))
    for name, v in tms.items():
        print(json.dumps({"path": name, "batch": 32, "hw": [576, 736], "ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                          "img_per_s": round(32e3 / statistics.median(v), 1)}))


if __name__ == "__main__":
    main()
