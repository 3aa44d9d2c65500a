"""What drawing into and cropping out of NV12 frames costs, on the SAME box and inputs as the RGB paths.  A record, not a gate.
Drawing: the workload of tools/render_bench.py -- 32 frames of 1080 x 1920, the reference's detections of bench.py's C2 workload (tests/golden/bench_c2.npz) scaled to
the frame -- through (a) render_nv12_kernel into the planes, (b) render_kernel into the same frames as interleaved RGB8, (c) the status-quo composition:
ops.nv12_to_rgb -> ops.draw_detections -> RGB -> NV12 in torch (BT.601 limited in float, 2 x 2 mean chroma: what a user writes today; its bytes differ from (a)'s).
Cropping: the workload of tools/crop_bench.py -- the same detections unscaled on 576 x 736 frames, 224 x 224 fp16 -- through crop_resize_nv12_kernel against
ops.nv12_to_rgb per frame + crop_resize_kernel<u8 HWC>.

    python tools/render_nv12_bench.py [--repeats 20]
prints one JSON line; times are device events around the calls (drawing: the C entry points on preallocated buffers for the two kernels, the ops for the composition;
cropping: the ops on both sides, their allocations inside the bracket), alternating the variants inside every repeat."""
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
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()

    import numpy as np
    import torch

    from yolort_amd import _lib, ops

    dev = torch.device("cuda:0")
    lib = _lib.load(require_gpu=True)
    z = np.load(args.golden)
    n, k, gh, gw = args.batch, 300, 576, 736

    def slab(h, w):
        boxes, scores, labels, counts = np.zeros((n, k, 4), np.float32), np.zeros((n, k), np.float32), np.zeros((n, k), np.int64), []
        for i in range(n):
            b = z[f"det{i % 8}_boxes"].astype(np.float32) * np.array([w / gw, h / gh, w / gw, h / gh], np.float32)
            boxes[i, :len(b)], scores[i, :len(b)], labels[i, :len(b)] = b, z[f"det{i % 8}_scores"], z[f"det{i % 8}_labels"]
            counts.append(len(b))
        return [torch.from_numpy(v).to(dev) for v in (boxes, scores, labels)] + [torch.tensor(counts, dtype=torch.int32, device=dev)], sum(counts)

    def timed(fns, repeats, warmup=2):
        """median / min / max ms per variant, the variants alternating inside every repeat"""
        ms = {name: [] for name in fns}
        for r in range(warmup + repeats):
            for name, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= warmup:
                    ms[name].append(e0.elapsed_time(e1))
        return {name: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for name, v in ms.items()}

    g = torch.Generator().manual_seed(1)
    frames = lambda h, w: [torch.randint(0, 256, (h * 3 // 2, w), generator=g, dtype=torch.uint8).to(dev) for _ in range(n)]   # noqa: E731

    # ---- drawing ----
    h, w = 1080, 1920
    (boxes, scores, labels, counts), total = slab(h, w)
    names = [f"class{i}" for i in range(80)]
    pristine = frames(h, w)
    nv = [f.clone() for f in pristine]
    rgb = [ops.nv12_to_rgb(f) for f in pristine]
    kw = dict(names=names, inplace=True)
    _, st = ops.draw_detections_nv12(nv, boxes, scores, labels, counts, **kw)     # also builds the cached tables
    assert st.tolist() == [0]
    lw, fs = ops.render_defaults(h, w)
    table, palette = ops._render_table("names", tuple(names), dev), ops._render_table("colors", tuple(v for row in ops.DEFAULT_COLORS for v in row), dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    arr = lambda vals, ty=C.c_int32: (ty * len(vals))(*vals)   # noqa: E731
    hw, lws, fss = arr([h, w] * n), arr([lw] * n), arr([fs] * n)
    ys, uvs, pitch, rgbs = arr([f.data_ptr() for f in nv], C.c_void_p), arr([f.data_ptr() + h * w for f in nv], C.c_void_p), arr([w, w] * n), arr([r.data_ptr() for r in rgb], C.c_void_p)
    dn, dr = _lib.RenderNv12Desc(), _lib.RenderDesc()
    for d in (dn, dr):
        d.hw, d.lw, d.fs = (C.cast(a, C.POINTER(C.c_int32)) for a in (hw, lws, fss))
        d.boxes, d.scores, d.labels, d.counts, d.status = boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), counts.data_ptr(), status.data_ptr()
        d.names, d.colors, d.m, d.num_classes, d.draw_labels, d.draw_conf, d.n, d.k = table.data_ptr(), palette.data_ptr(), 20, 80, 1, 1, n, k
        for i in range(3):
            d.txt_color[i] = 255
    dn.y, dn.uv, dn.pitch = C.cast(ys, C.POINTER(C.c_void_p)), C.cast(uvs, C.POINTER(C.c_void_p)), C.cast(pitch, C.POINTER(C.c_int32))
    dr.imgs, dr.in_dtype = C.cast(rgbs, C.POINTER(C.c_void_p)), _lib.YMI_U8_HWC

    def rgb_to_nv12(im):
        """the torch composition a user writes today: BT.601 limited in float, chroma = the mean of the 2 x 2 block"""
        r, g_, b = im[..., 0].float(), im[..., 1].float(), im[..., 2].float()
        y = 16 + (65.481 * r + 128.553 * g_ + 24.966 * b) / 255
        cb, cr = 128 + (-37.797 * r - 74.203 * g_ + 112.0 * b) / 255, 128 + (112.0 * r - 93.786 * g_ - 18.214 * b) / 255
        c = torch.stack([cb, cr], -1).reshape(h // 2, 2, w // 2, 2, 2).mean((1, 3)).reshape(h // 2, w)
        return torch.cat([y, c]).round().clamp(0, 255).to(torch.uint8)

    def compose():
        out, _ = ops.draw_detections([ops.nv12_to_rgb(f) for f in pristine], boxes, scores, labels, counts, **kw)
        return [rgb_to_nv12(im) for im in out]

    res = {"gpu": torch.cuda.get_device_name(0), "frames": n, "frame_hw": [h, w], "boxes": total, "lw": lw, "fs": fs}
    res["draw_ms"] = timed({"render_nv12_kernel": lambda: _lib.check(lib.ymi_render_nv12(C.byref(dn), _lib.stream_ptr()), "ymi_render_nv12"),
                            "render_kernel_rgb8": lambda: _lib.check(lib.ymi_render(C.byref(dr), _lib.stream_ptr()), "ymi_render"),
                            "nv12_to_rgb+draw+torch_rgb_to_nv12": compose}, args.repeats)
    m = {name: v["median"] for name, v in res["draw_ms"].items()}
    res["nv12_over_rgb8_kernel"] = round(m["render_nv12_kernel"] / m["render_kernel_rgb8"], 3)
    res["composition_over_nv12_kernel"] = round(m["nv12_to_rgb+draw+torch_rgb_to_nv12"] / m["render_nv12_kernel"], 1)
    changed = [a != b for a, b in zip(nv, pristine)]
    res["bytes_changed"] = {"y": sum(int(c[:h].sum()) for c in changed), "uv": sum(int(c[h:].sum()) for c in changed), "rgb8_of_the_same_pixels": 3 * sum(int(c[:h].sum()) for c in changed)}

    # ---- cropping ----
    h, w = gh, gw
    (boxes, _, _, counts), total = slab(h, w)
    fr = frames(h, w)
    size = (224, 224)
    crops, index, tot = ops.crop_detections_nv12(fr, boxes, counts, size, capacity=total)
    want = ops.crop_detections([ops.nv12_to_rgb(f) for f in fr], boxes, counts, size, capacity=total)
    assert tot.tolist() == [total, 0] and torch.equal(crops, want[0]) and torch.equal(index, want[1])   # bit for bit at the size that is timed
    res["crop"] = {"frame_hw": [h, w], "size": list(size), "dtype": "fp16", "crops": total}
    res["crop_ms"] = timed({"crop_resize_nv12_kernel": lambda: ops.crop_detections_nv12(fr, boxes, counts, size, capacity=total),
                            "nv12_to_rgb+crop_resize_kernel": lambda: ops.crop_detections([ops.nv12_to_rgb(f) for f in fr], boxes, counts, size, capacity=total)}, args.repeats)
    res["crop_composition_over_nv12"] = round(res["crop_ms"]["nv12_to_rgb+crop_resize_kernel"]["median"] / res["crop_ms"]["crop_resize_nv12_kernel"]["median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
