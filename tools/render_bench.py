"""What drawing a batch's detections into its images costs: ymi_render (one render_kernel launch, in place) against the status quo on the SAME box and inputs -- the
images copied to the host, per box one PIL ImageDraw.rectangle (outline) + rectangle (label background) + text with Pillow's built-in font, the images copied back.
Inputs: 32 interleaved uint8 images of 1080 x 1920 and the reference's detections of bench.py's C2 workload (tests/golden/bench_c2.npz: 8 images of 576 x 736; image i of
the batch takes golden image i % 8, as tools/crop_bench.py tiles them), the boxes scaled to the image.  A record, not a gate.

    python tools/render_bench.py [--repeats 20] [--host-repeats 2]
prints one JSON line: kernel time per batch (device events around the launch), the host loop's time, the ratio, and the bytes of the tiles the kernel touches over its
time against the library's copy kernel (ymi_copy_view) on the same byte count."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--golden", default=os.path.join(ROOT, "tests", "golden", "bench_c2.npz"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()

    import numpy as np
    import torch
    from PIL import Image, ImageDraw, ImageFont

    from yolort_amd import _lib, ops

    dev = torch.device("cuda:0")
    z = np.load(args.golden)
    n, k = args.batch, 300
    h, w, gh, gw = 1080, 1920, 576, 736
    boxes, scores, labels, counts = np.zeros((n, k, 4), np.float32), np.zeros((n, k), np.float32), np.zeros((n, k), np.int64), []
    for i in range(n):
        b = z[f"det{i % 8}_boxes"].astype(np.float32) * np.array([w / gw, h / gh, w / gw, h / gh], np.float32)
        c = len(b)
        boxes[i, :c], scores[i, :c], labels[i, :c] = b, z[f"det{i % 8}_scores"], z[f"det{i % 8}_labels"]
        counts.append(c)
    total = sum(counts)
    g = torch.Generator().manual_seed(1)
    pristine = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(n)]
    images = [im.clone() for im in pristine]
    names = [f"class{i}" for i in range(80)]
    lw, fs = ops.render_defaults(h, w)
    t = dict(boxes=torch.from_numpy(boxes), scores=torch.from_numpy(scores), labels=torch.from_numpy(labels), counts=torch.tensor(counts, dtype=torch.int32))
    t = {f: v.to(dev) for f, v in t.items()}

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

    # the kernel: the C entry point directly, as the op calls it, on fixed buffers (drawing twice draws the same pixels: the repeats do the same work)
    out, status = ops.draw_detections(images, t["boxes"], t["scores"], t["labels"], t["counts"], names=names, inplace=True)
    torch.cuda.synchronize()
    assert status.tolist() == [0], status.tolist()
    lib = _lib.load(require_gpu=True)
    d = _lib.RenderDesc()
    ptrs, hw = (C.c_void_p * n)(*[im.data_ptr() for im in images]), (C.c_int32 * (2 * n))(*([h, w] * n))
    lws, fss = (C.c_int32 * n)(*([lw] * n)), (C.c_int32 * n)(*([fs] * n))
    table, palette = ops._render_table("names", tuple(names), dev), ops._render_table("colors", tuple(v for row in ops.DEFAULT_COLORS for v in row), dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    d.imgs, d.hw, d.lw, d.fs = C.cast(ptrs, C.POINTER(C.c_void_p)), C.cast(hw, C.POINTER(C.c_int32)), C.cast(lws, C.POINTER(C.c_int32)), C.cast(fss, C.POINTER(C.c_int32))
    d.boxes, d.scores, d.labels, d.counts, d.status = t["boxes"].data_ptr(), t["scores"].data_ptr(), t["labels"].data_ptr(), t["counts"].data_ptr(), st.data_ptr()
    d.names, d.colors, d.m, d.num_classes, d.in_dtype, d.draw_labels, d.draw_conf, d.n, d.k = table.data_ptr(), palette.data_ptr(), 20, 80, _lib.YMI_U8_HWC, 1, 1, n, k
    for i in range(3):
        d.txt_color[i] = 255
    med, lo, hi = timed(lambda: _lib.check(lib.ymi_render(C.byref(d), _lib.stream_ptr()), "ymi_render"), args.repeats)
    changed = [(a != b).any(-1) for a, b in zip(images, pristine)]
    # the tiles the kernel touches: 64 x 16 tiles with at least one changed pixel (a lower bound: a covered pixel may keep its value by chance, 1 in 2^24)
    tiles = sum(int(torch.nn.functional.max_pool2d(c[None, None].float(), (16, 64), ceil_mode=True).sum()) for c in changed)
    pixels = sum(int(c.sum()) for c in changed)
    tile_bytes = tiles * 64 * 16 * 3
    res = {"gpu": torch.cuda.get_device_name(0), "images": n, "image_hw": [h, w], "layout": "uint8 HWC", "boxes": total, "lw": lw, "fs": fs, "tiles_touched": tiles,
           "tiles_all": n * ((h + 15) // 16) * ((w + 63) // 64), "pixels_drawn": pixels, "kernel_ms": {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)},
           "touched_tile_bytes": tile_bytes, "touched_tile_TBps": round(tile_bytes / (med * 1e-3) / 1e12, 4), "pixel_bytes_TBps": round(pixels * 3 / (med * 1e-3) / 1e12, 4)}

    # store-rate yardstick: the library's copy kernel on the same byte count
    npix = max(tile_bytes // 128, 1)
    src, dst = torch.empty(npix * 64, dtype=torch.float16, device=dev).normal_(), torch.empty(npix * 64, dtype=torch.float16, device=dev)
    cm, _, _ = timed(lambda: _lib.check(lib.ymi_copy_view(src.data_ptr(), 64, npix, 64, dst.data_ptr(), 64, _lib.YMI_F16, _lib.stream_ptr()), "ymi_copy_view"), args.repeats)
    res["copy_view_ms"], res["copy_view_write_TBps"] = round(cm, 4), round(npix * 128 / (cm * 1e-3) / 1e12, 3)
    res["kernel_over_copy_rate"] = round(res["touched_tile_TBps"] / res["copy_view_write_TBps"], 4)

    # the status quo: device -> host, a PIL loop in the reference's order (reversed: the first detection ends on top), host -> device
    font = ImageFont.load_default_imagefont()
    colours = [tuple(c) for c in ops.DEFAULT_COLORS]
    th = 11 * fs

    def host_loop():
        back = []
        for i, im in enumerate(pristine):
            pil = Image.fromarray(im.cpu().numpy())
            draw = ImageDraw.Draw(pil)
            for j in reversed(range(counts[i])):
                x0, y0, x1, y1 = (int(v) for v in boxes[i, j])
                if x1 < x0 or y1 < y0:
                    continue
                colour = colours[int(labels[i, j]) % 20]
                text = f"{names[int(labels[i, j])]} {float(scores[i, j]):.2f}"
                draw.rectangle([x0, y0, x1, y1], width=lw, outline=colour)
                tw = 6 * len(text)                # (the built-in font is not magnified here: the status quo draws SMALLER text for the same calls)
                ty = y0 - th if y0 - th >= 0 else y0
                draw.rectangle([x0, ty, x0 + tw * fs + 1, ty + th + 1], fill=colour)
                draw.text((x0, ty), text, fill=(255, 255, 255), font=font)
            back.append(torch.from_numpy(np.asarray(pil)).to(dev))
        torch.cuda.synchronize()
        return back

    host_ms = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        back = host_loop()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    res["host_loop_ms"] = {"median": round(statistics.median(host_ms), 1), "min": round(min(host_ms), 1), "max": round(max(host_ms), 1)}
    res["ratio_host_over_kernel"] = round(statistics.median(host_ms) / med, 1)
    # outlines and backgrounds of the two agree wherever the text (not magnified on the host, overlapping glyphs in ImageDraw.text) is not: report, do not assert
    res["fraction_of_drawn_pixels_equal_to_host"] = round(float(sum(int(((a == b).all(-1) & c).sum()) for a, b, c in zip(images, back, changed))) / max(pixels, 1), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
