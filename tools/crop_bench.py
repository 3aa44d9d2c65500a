"""What cutting a batch's detections out of its images costs: ops.crop_detections (one crop_resize_kernel launch) against the status-quo composition on the SAME device
and inputs -- the rectangles known on the host, one F.interpolate(mode="bilinear", align_corners=False) per box on the device written into the same output buffer (no
.cpu() round trip of pixels).  Inputs: the reference's detections of bench.py's C2 workload (tests/golden/bench_c2.npz: 8 images; image i of the 32-image batch takes
golden image i % 8) on seeded 576 x 736 fp16 images, cropped to 224 x 224 fp16 with save_one_box's defaults.  A record, not a gate.

    python tools/crop_bench.py [--repeats 20] [--compose-repeats 3]
prints one JSON line: kernel time per batch (device events around the launch) for the four-pixels-per-thread mapping and for one pixel per thread
(YOLORT_AMD_CROP=pixel), bytes written per second, the same bytes through the library's copy kernel (ymi_copy_view) and torch's fill, the composition's time, the ratio."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--golden", default=os.path.join(ROOT, "tests", "golden", "bench_c2.npz"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--compose-repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, nargs=2, default=(224, 224))
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F

    from workloads.synth import synth_images
    from yolort_amd import _lib, ops

    dev = torch.device("cuda:0")
    z = np.load(args.golden)
    n, k = args.batch, 300
    h, w = 576, 736
    boxes = np.zeros((n, k, 4), np.float32)
    counts = []
    for i in range(n):
        b = z[f"det{i % 8}_boxes"]
        boxes[i, : len(b)] = b
        counts.append(len(b))
    total = sum(counts)
    images = [im.contiguous() for im in synth_images(n, h, w, seed=1).to(dev).half()]
    slab, cnt = torch.from_numpy(boxes).to(dev), torch.tensor(counts, dtype=torch.int32, device=dev)
    size = tuple(args.size)

    def timed(fn, repeats, warmup=2):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    # the kernel: outputs allocated once (the op's own torch.empty calls would be inside the bracket otherwise) -> the C entry point directly, as the op calls it
    crops, index, tot = ops.crop_detections(images, slab, cnt, size, capacity=total)
    torch.cuda.synchronize()
    assert tot.tolist() == [total, 0], tot.tolist()
    nbytes = crops.numel() * crops.element_size()
    lib = _lib.load(require_gpu=True)
    scratch_out, scratch_index, scratch_total = torch.empty_like(crops), torch.empty_like(index), torch.empty_like(tot)
    d = _lib.CropDesc()
    ptrs, hw = (C.c_void_p * n)(*[im.data_ptr() for im in images]), (C.c_int32 * (2 * n))(*([h, w] * n))
    d.imgs, d.hw = C.cast(ptrs, C.POINTER(C.c_void_p)), C.cast(hw, C.POINTER(C.c_int32))
    d.boxes, d.counts, d.crops, d.index, d.total = slab.data_ptr(), cnt.data_ptr(), scratch_out.data_ptr(), scratch_index.data_ptr(), scratch_total.data_ptr()
    d.gain, d.pad, d.n, d.k, d.cap, d.out_h, d.out_w, d.in_dtype, d.out_dtype = 1.02, 10.0, n, k, total, size[0], size[1], _lib.YMI_F16, _lib.YMI_F16
    res = {"gpu": torch.cuda.get_device_name(0), "images": n, "image_hw": [h, w], "boxes": total, "size": list(size), "dtype": "float16", "bytes_written": nbytes}
    for name, env in (("kernel_4px", None), ("kernel_1px", "pixel")):
        if env is None:
            os.environ.pop("YOLORT_AMD_CROP", None)
        else:
            os.environ["YOLORT_AMD_CROP"] = env
        med, lo, hi = timed(lambda: _lib.check(lib.ymi_crop_resize(C.byref(d), _lib.stream_ptr()), "ymi_crop_resize"), args.repeats)
        res[name + "_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
        res[name + "_TBps"] = round(nbytes / (med * 1e-3) / 1e12, 3)
        torch.cuda.synchronize()
        res[name + "_equal"] = bool(torch.equal(scratch_out, crops)) and bool(torch.equal(scratch_index, index))
    os.environ.pop("YOLORT_AMD_CROP", None)

    # store-rate yardsticks on the same buffer size: the library's copy kernel and torch's fill
    src = scratch_out
    npix = nbytes // 128
    med, lo, hi = timed(lambda: _lib.check(lib.ymi_copy_view(crops.data_ptr(), 64, npix, 64, src.data_ptr(), 64, _lib.YMI_F16, _lib.stream_ptr()), "ymi_copy_view"), args.repeats)
    res["copy_view_ms"], res["copy_view_write_TBps"] = round(med, 4), round(nbytes / (med * 1e-3) / 1e12, 3)
    med, lo, hi = timed(lambda: src.fill_(0.5), args.repeats)
    res["torch_fill_ms"], res["torch_fill_TBps"] = round(med, 4), round(nbytes / (med * 1e-3) / 1e12, 3)

    # the composition: rectangles on the host (one download of the index, outside the bracket), one F.interpolate per box into the same kind of buffer
    crops2 = crops
    rows = index.cpu().tolist()
    wide = images
    dst = scratch_out.zero_()

    def compose():
        for r, (i, _, x1, y1, x2, y2) in enumerate(rows):
            if x2 > x1 and y2 > y1:
                dst[r] = F.interpolate(wide[i][None, :, y1:y2, x1:x2].float(), size=size, mode="bilinear", align_corners=False)[0]

    med, lo, hi = timed(compose, args.compose_repeats, warmup=1)
    res["compose_ms"] = {"median": round(med, 2), "min": round(lo, 2), "max": round(hi, 2)}
    res["compose_max_abs_diff"] = float((dst.float() - crops2.float()).abs().max())
    res["ratio_compose_over_kernel"] = round(med / res["kernel_4px_ms"]["median"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
