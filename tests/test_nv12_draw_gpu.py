"""NV12 drawing and cropping on the GPU (csrc/preproc_nv12.hip): render_nv12_kernel against the painter of tests/_render_cases.py bit for bit (guard bands, base
offsets and pitch padding included), its refusals and a captured graph; crop_resize_nv12_kernel against ymi_crop_resize on the converted frames; the Python frame
forms and the YOLOv5 convenience methods against their own composition.  Yardsticks and cases: tests/_nv12draw_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _nv12draw_cases as D
from _nv12_cases import TABLES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from yolort_amd import _lib
    return _lib.load(require_gpu=True)


@pytest.mark.parametrize("name", list(D.CASES))
def test_render_nv12_equals_the_painter_bit_for_bit(dev, lib, name):
    D.check(lib, D.CASES[name], dev)


@pytest.mark.parametrize("matrix,full", TABLES)
def test_render_nv12_under_every_matrix_and_range(dev, lib, matrix, full):
    D.check(lib, D.CASES["overlap"]._replace(matrix=matrix, full=full), dev)


def test_refusals_launch_nothing(dev, lib):
    D.check_refusals(lib, dev)


def test_graph_capture_and_three_replays(dev, lib):
    nd = D.CASES["overlap"]
    d, bufs, status, keep = D.describe(nd, dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        assert lib.ymi_render_nv12(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    D.compare(nd, bufs, status, want="input")      # capturing draws nothing
    first = [b.clone() for b in bufs]
    for _ in range(3):
        for b, f in zip(bufs, first):
            b.copy_(f)
        status.copy_(torch.tensor([-77, 0, -77], dtype=torch.int32))   # the caller zeroes the status word
        graph.replay()
        torch.cuda.synchronize()
        D.compare(nd, bufs, status)                # == the eager result, which is the painter's


# ---- crop ------------------------------------------------------------------------------------------------------------------------------------------------------------
CROP_SIZES = ((2, 2), (6, 10), (18, 34), (40, 66))


def _pitched_pairs(dev):
    """ragged frames as (y, uv) views with a pitch above the width, the Y base one byte and the chroma base two bytes into their allocations"""
    g, out = torch.Generator().manual_seed(3), []
    for h, w in CROP_SIZES:
        y, uv = (torch.randint(0, 256, (o + r * (w + 6),), generator=g, dtype=torch.uint8).to(dev).as_strided((r, w), (w + 6, 1), o) for r, o in ((h, 1), (h // 2, 2)))
        out.append((y, uv))
    return out


def _crop_slab(dev):
    """per frame: a box over the top-left corner, one over the bottom-right corner, the whole frame, an empty box, a non-finite one"""
    rows = [[(-3, -3, w / 2, h / 2), (w / 2 - 1, h / 2 - 1, w + 5, h + 5), (0, 0, w, h), (1, 1, 1, 5), (float("nan"), 0, w, float("inf"))] for h, w in CROP_SIZES]
    return torch.tensor(rows, dtype=torch.float32, device=dev), torch.tensor([5, 4, 5, 5], dtype=torch.int32, device=dev)


@pytest.mark.parametrize("size", [(8, 8), (5, 7)], ids=["wide", "scalar"])
@pytest.mark.parametrize("kw", [dict(), dict(square=True, dtype=torch.float32), dict(mean=(0.4, 0.5, 0.6), std=(0.2, 0.3, 0.25), dtype=torch.bfloat16), dict(capacity=7),
                                dict(matrix="bt709", full_range=True)], ids=["default", "square-f32", "meanstd-bf16", "capacity", "bt709-full"])
def test_crop_nv12_equals_crop_of_the_converted_frames(dev, size, kw):
    from yolort_amd import _lib, ops
    frames, (boxes, counts) = _pitched_pairs(dev), _crop_slab(dev)
    conv = {k: kw[k] for k in ("matrix", "full_range") if k in kw}
    got = ops.crop_detections_nv12(frames, boxes, counts, size, **kw)
    want = ops.crop_detections([ops.nv12_to_rgb(f, **conv) for f in frames], boxes, counts, size, **{k: v for k, v in kw.items() if k not in conv})
    total = want[2].tolist()
    assert got[2].tolist() == total == ([7, _lib.CROP_STATUS_CAPACITY] if "capacity" in kw else [19, 0])
    assert torch.equal(got[1][:total[0]], want[1][:total[0]]) and torch.equal(got[0][:total[0]].view(torch.uint8), want[0][:total[0]].view(torch.uint8))
    assert got[0][:total[0]].float().abs().sum() > 0


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------------------------------
def test_frame_forms_and_convenience_methods_equal_their_composition(dev):
    """packed frames and pitched pairs through ops.draw_detections_nv12 (copies come back packed, inplace draws into the planes handed in); YOLOv5.render_nv12 /
    crop_nv12 on a golden photo equal the ops called on the slab of forward_nv12's detections"""
    from PIL import Image
    from workloads.synth import synth_weights
    from yolort_amd import ops
    from yolort_amd.models import YOLOv5
    pairs = _pitched_pairs(dev)[2:]
    boxes, counts = torch.tensor([[[2, 3, 30, 15]], [[5, 13, 60, 38]]], dtype=torch.float32, device=dev), torch.tensor([1, 1], dtype=torch.int32, device=dev)
    scores, labels = torch.full((2, 1), 0.5, device=dev), torch.tensor([[1], [2]], device=dev)
    packed = [torch.cat([y, uv]) for y, uv in pairs]
    before = [(y.clone(), uv.clone()) for y, uv in pairs]
    out, status = ops.draw_detections_nv12(pairs, boxes, scores, labels, counts, names=["a", "b", "c"])
    ref, _ = ops.draw_detections_nv12(packed, boxes, scores, labels, counts, names=["a", "b", "c"])
    assert status.item() == 0 and all(o.is_contiguous() and torch.equal(o, r) and not torch.equal(o, p) for o, r, p in zip(out, ref, packed))
    assert all(torch.equal(y, by) and torch.equal(uv, buv) for (y, uv), (by, buv) in zip(pairs, before)), "inplace=False leaves the input planes alone"
    same, _ = ops.draw_detections_nv12(pairs, boxes, scores, labels, counts, names=["a", "b", "c"], inplace=True)
    assert all(s is p and torch.equal(torch.cat(list(p)), o) for s, p, o in zip(same, pairs, out))
    with pytest.raises(ValueError):
        ops.draw_detections_nv12([packed[0][:, :33]], boxes[:1], scores[:1], labels[:1], counts[:1])
    arch = "yolov5_darknet_pan_n_r60"
    m = YOLOv5(arch=arch, size=(192, 320), score_thresh=0.05)
    m.load_state_dict(synth_weights(m.state_dict(), arch, seed=0, head_gain=1.0))
    m = m.to(dev).half().eval()
    photo = np.asarray(Image.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zidane.png")).convert("RGB"))[::2, ::2]   # 360 x 640
    as_nv12 = lambda rgb: np.concatenate([rgb[..., 1], np.stack([rgb[::2, ::2, 2], rgb[::2, ::2, 0]], -1).reshape(rgb.shape[0] // 2, rgb.shape[1])])   # noqa: E731
    frames = [torch.from_numpy(as_nv12(p)).to(dev) for p in (photo, photo[40:300, 100:520])]
    dets = m.forward_nv12(frames)
    slab = m._slab(dets, 2, dev, "test")
    assert sum(slab[4]) > 0
    want, _ = ops.draw_detections_nv12(frames, *slab[:4], matrix="bt709")
    assert all(torch.equal(a, b) for a, b in zip(m.render_nv12(frames, dets, matrix="bt709"), want)) and not torch.equal(want[0], frames[0])
    crops, _, _ = ops.crop_detections_nv12(frames, slab[0], slab[3], (32, 32), capacity=sum(slab[4]))
    assert torch.equal(torch.cat(m.crop_nv12(frames, size=(32, 32))), crops)
