"""NV12 ingest on the GPU (csrc/preproc_nv12.hip): the conversion against the integer rule and the real-valued formula on the grid frame, the fused letterbox on raw bits
under every kernel variant, its equivalence with ymi_letterbox on the converted image, the Python frame forms and refusals, and forward_nv12 against forward on the
converted frames.  Cases and yardsticks: tests/_nv12_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _nv12_cases as N
from _pre_cases import DT_CODE, FILL, LB_VARIANTS, TORCH_DT, bits

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from yolort_amd import _lib
    return _lib.load(require_gpu=True)


def _packed(y, uv, dev):
    return torch.from_numpy(np.concatenate([y, uv])).to(dev)


@pytest.mark.parametrize("matrix,full", N.TABLES)
def test_conversion_is_the_integer_rule_within_the_derived_bound_of_the_real_one(dev, matrix, full):
    from yolort_amd import ops
    y, uv = N.grid_frame()
    got = ops.nv12_to_rgb(_packed(y, uv, dev), matrix=matrix, full_range=full).cpu().numpy()
    assert np.array_equal(got, N.convert_int(y, uv, matrix, full))
    real = N.convert_real(y, uv, matrix, full)
    err = np.abs(got - np.clip(real, 0, 255)).max()
    print(f"{matrix} full={full}: max |codes - real formula| = {err:.5f}, bound {N.CONVERT_BOUND:.5f}")
    assert err <= N.CONVERT_BOUND and (real < 0).any() and (real > 255).any()   # both clamps occur in the frame


@pytest.mark.parametrize("name", [c.name for c in N.CASES])
def test_letterbox_nv12_equals_the_model_bit_for_bit(dev, lib, name):
    """every kernel variant (default, pixel, rows per wave 1 / 2 / 4 x column groups 1 / 2) equals the model on raw bits, pads and zero channels included"""
    outs = N.check(lib, N.BY_NAME[name], dev)
    assert set(outs) == {v[0] for v in LB_VARIANTS}


@pytest.mark.parametrize("name", ["scales", "pitch", "misaligned"])
def test_letterbox_nv12_equals_ymi_letterbox_of_the_converted_frames(dev, lib, name):
    """pair frames (pitched views at their own alignments) through ops.letterbox_nv12 == ymi_letterbox(YMI_U8_HWC) of ops.nv12_to_rgb's images, bit for bit"""
    from yolort_amd import ops
    case = N.BY_NAME[name]
    pairs = []
    for (y, uv), f in zip(N.frames(case), case.frames):
        ty, tuv = (torch.cat([torch.zeros(o, dtype=torch.uint8), torch.from_numpy(p).reshape(-1)]).to(dev).as_strided((p.shape[0], f[1]), (p.shape[1], 1), o)
                   for p, o in ((y, f[8]), (uv, f[9])))   # views with the case's pitch, their base `o` bytes past the allocation's
        pairs.append((ty, tuv))
    sizes, pads = [f[2:4] for f in case.frames], [f[4:6] for f in case.frames]
    kw = dict(matrix=case.matrix, full_range=case.full)
    got = ops.letterbox_nv12(pairs, sizes, pads, (case.hb, case.wb), dtype=TORCH_DT[case.out_dt], **kw)
    rgbs = [ops.nv12_to_rgb(p, **kw) for p in pairs]
    assert all(np.array_equal(r.cpu().numpy(), N.rgb8(case, i)) for i, r in enumerate(rgbs))
    want = torch.empty_like(got)
    ptrs = (C.c_void_p * len(rgbs))(*[r.data_ptr() for r in rgbs])
    geom = (C.c_int32 * (6 * len(rgbs)))(*[v for f in case.frames for v in f[:6]])
    assert lib.ymi_letterbox(ptrs, geom, len(rgbs), 4, want.data_ptr(), case.hb, case.wb, 4, DT_CODE[case.out_dt], C.c_float(FILL), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(got.cpu()), bits(want.cpu())) and torch.equal(bits(got.cpu()), bits(N.model(case)))
    packed = ops.letterbox_nv12([_packed(y[:, :f[1]], uv[:, :f[1]], dev) for (y, uv), f in zip(N.frames(case), case.frames)], sizes, pads, (case.hb, case.wb),
                                dtype=TORCH_DT[case.out_dt], **kw)
    assert torch.equal(bits(packed.cpu()), bits(want.cpu()))


def test_refusals(dev, lib):
    from yolort_amd import ops
    from yolort_amd.models import YOLOv5
    N.check_refusals(lib, dev)
    ok = torch.zeros(12, 16, dtype=torch.uint8, device=dev)
    for bad in (ok.float(), ok[:11], ok[:, :15], ok[:, ::2], ok.cpu()[None], (ok[:8], ok[8:, :14]), (ok[:8], ok[8:11]), (ok[:8, 1:15], ok[8:, 1:15]), (ok[:8],)):
        with pytest.raises(ValueError):
            ops.nv12_to_rgb(bad)
    with pytest.raises(ValueError):
        ops.nv12_to_rgb(ok, matrix="bt2020")
    with pytest.raises(ValueError):
        ops.letterbox_nv12([ok], [(8, 16)], [(0, 0)], (8, 16), dtype=torch.float64)
    m = YOLOv5(arch="yolov5_darknet_pan_n_r60", size=(160, 160)).to(dev).half().eval()
    with pytest.raises(ValueError):
        m([ok])                                     # forward() keeps refusing a 2-D tensor: NV12 goes through forward_nv12
    with pytest.raises(ValueError):
        m.forward_nv12([ok[:11]])


def _as_nv12(rgb):
    """(h, w, 3) uint8 -> a packed NV12 buffer with the photo's structure (G as luma, subsampled B / R as chroma): test input only, no inverse of the contract"""
    return np.concatenate([rgb[..., 1], np.stack([rgb[::2, ::2, 2], rgb[::2, ::2, 0]], -1).reshape(rgb.shape[0] // 2, rgb.shape[1])])


@pytest.mark.parametrize("half", [True, False], ids=["fp16", "fp32"])
def test_forward_nv12_returns_the_detections_of_forward_on_the_converted_frames(dev, half):
    """yolov5n on a golden photo (and a crop of it: two sizes in the batch), three batches: the plan's graph is captured at the first and replayed after it"""
    from PIL import Image
    from workloads.synth import synth_weights
    from yolort_amd import ops
    from yolort_amd.models import YOLOv5
    arch = "yolov5_darknet_pan_n_r60"
    m = YOLOv5(arch=arch, size=(192, 320), score_thresh=0.05)
    m.load_state_dict(synth_weights(m.state_dict(), arch, seed=0, head_gain=1.0))
    m = (m.to(dev).half() if half else m.to(dev)).eval()
    photo = np.asarray(Image.open(os.path.join(GOLD, "zidane.png")).convert("RGB"))[::2, ::2]   # 360 x 640
    frames = [torch.from_numpy(_as_nv12(p)).to(dev) for p in (photo, photo[40:300, 100:520])]
    want = m([ops.nv12_to_rgb(f) for f in frames])
    assert m.model.use_graph and sum(len(d["scores"]) for d in want) > 0
    for _ in range(3):
        got = m.forward_nv12(frames)
        for a, b in zip(want, got):
            assert all(torch.equal(a[k], b[k]) for k in ("boxes", "scores", "labels"))
