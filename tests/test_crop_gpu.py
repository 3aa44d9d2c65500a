"""Detection crops (include/yolort_amd.h ymi_crop_resize, Python `ops.crop_detections` / `YOLOv5.crop`) on the GPU: the cases of tests/test_crop.py on the real kernel
(same inputs, same expectations, poisoned guard bands around both outputs), the public op bit for bit against the driver's run, graph capture and replay with
changed counts, and YOLOv5.crop on a model's own detections.  Yardsticks and cases: tests/_crop_cases.py."""
import pytest
import torch

import _crop_cases as T
import test_crop as CPU

pytestmark = pytest.mark.gpu
ARCH, SEED, CANVAS = "yolov5_darknet_pan_n_r60", 7, (128, 160)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from yolort_amd import _lib
    return _lib.load(require_gpu=True)


def _op(case, dev, **kw):
    """ops.crop_detections of a case -> (crops fp32 on the host, index, total)"""
    from yolort_amd import ops
    images = [im.to(dev) for im in case.images]
    crops, index, total = ops.crop_detections(images, torch.from_numpy(case.boxes).to(dev), torch.tensor(case.counts, dtype=torch.int32, device=dev), case.size,
                                              gain=case.gain, pad=case.pad, square=case.square, mean=case.mean, std=case.std, dtype=T.TORCH_DT[case.out_dt], **kw)
    assert crops.is_cuda and index.is_cuda and total.is_cuda and crops.dtype == T.TORCH_DT[case.out_dt] and index.dtype == total.dtype == torch.int32
    return crops.float().cpu(), index.cpu(), total.cpu()


def _run_both(lib, dev, case):
    """the driver's run between guard bands, checked against the yardsticks; then the public op, whose rows below the total equal the driver's bit for bit"""
    out = T.run_crop(lib, case, dev)
    T.check_crop(out, case)
    crops, index, total = _op(case, dev, capacity=case.cap)
    w = int(total[0])
    assert total.tolist() == out["total"].tolist() and tuple(crops.shape) == (case.cap, 3) + case.size and tuple(index.shape) == (case.cap, 6)
    assert torch.equal(crops[:w], out["crops"][:w]) and torch.equal(index[:w], out["index"][:w])
    return out


# ---- rectangles ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gi", range(5))
def test_library_rectangles_equal_the_reference_rectangles(dev, lib, gi):
    CPU._golden_case(lib, gi, dev)


# ---- pixels --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,in_dt,out_dt", CPU.EXACT, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_power_of_two_weights_are_bit_exact(dev, lib, size, in_dt, out_dt):
    _run_both(lib, dev, T.exact_case(size, in_dt, out_dt))


def test_normalised_identity_is_bit_exact(dev, lib):
    _run_both(lib, dev, T.exact_case((8, 8), "u8hwc", "f32", *T.IMAGENET))


@pytest.mark.parametrize("out_dt", T.OUT_DTS)
def test_up_and_down_scaling(dev, lib, out_dt):
    _run_both(lib, dev, T.scaling_case(out_dt))


@pytest.mark.parametrize("size", T.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("params", [dict(), dict(square=True, gain=1.3, pad=30), dict(mean=T.IMAGENET[0], std=T.IMAGENET[1]), dict(out_dt="f16", mean=T.IMAGENET[0], std=T.IMAGENET[1])],
                         ids=["save_one_box", "apply_classifier", "normalised", "normalised-f16"])
def test_ragged_counts(dev, lib, size, params):
    _run_both(lib, dev, T.ragged(size, **params))


@pytest.mark.parametrize("in_dt", T.IN_DTS)
@pytest.mark.parametrize("out_dt", T.OUT_DTS)
def test_every_input_and_output_dtype(dev, lib, in_dt, out_dt):
    _run_both(lib, dev, T.ragged((8, 8), in_dt=in_dt, out_dt=out_dt))


# ---- layout and bookkeeping ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(8, 8), (7, 5)], ids=["wide", "scalar"])
def test_66_images_cross_the_launch_boundary_with_global_offsets(dev, lib, size):
    case = T.many_images_case(size)
    out = _run_both(lib, dev, case)
    assert out["index"][case.total - 3: case.total, 0].tolist() == [65, 65, 65]


def test_capacity_equal_below_and_zero(dev, lib):
    CPU._capacity_cases(lib, dev)
    case = T.ragged((8, 8))
    crops, index, total = _op(case, dev)                      # the default capacity is n * K
    assert tuple(crops.shape) == (len(case.sizes) * T.K, 3, 8, 8) and total.tolist() == [case.total, 0]
    crops, index, total = _op(case, dev, capacity=0)
    assert tuple(crops.shape) == (0, 3, 8, 8) and tuple(index.shape) == (0, 6) and total.tolist() == [0, T.STATUS_CAPACITY]


def test_count_above_k_or_negative_sets_the_status_bit(dev, lib):
    CPU._bad_count_cases(lib, dev)


def test_non_finite_boxes_give_zero_crops(dev, lib):
    out = _run_both(lib, dev, T.nonfinite_case())
    assert [r == [0, 0, 0, 0] for r in out["index"][:8, 2:].tolist()] == [True, True, True, False, True, True, False, True]


def test_empty_batch_and_empty_slab(dev, lib):
    for case in (T.Case("no-images", [], [], (8, 8), cap=3), T.Case("no-detections", [(8, 8), (8, 8)], [0, 0], (8, 8), cap=3)):
        out = T.run_crop(lib, case, dev)
        T.check_crop(out, case)
        assert out["total"].tolist() == [0, 0]


def test_refusals(dev, lib):
    from yolort_amd import ops
    from yolort_amd._lib import YmiError
    T.check_refusals(lib, dev)
    case = T.ragged((8, 8))
    images, boxes, counts = [im.to(dev) for im in case.images], torch.from_numpy(case.boxes).to(dev), torch.tensor(case.counts, dtype=torch.int32, device=dev)
    for kw in (dict(size=(0, 8)), dict(size=(8, 8), capacity=-1), dict(size=(8, 8), dtype=torch.float64), dict(size=(8, 8), mean=(0, 0, 0), std=(1, 0, 1)),
               dict(size=(8, 8), gain=float("nan")), dict(size=(8, 8), pad=float("inf"))):
        with pytest.raises(YmiError):
            ops.crop_detections(images, boxes, counts, **kw)
    with pytest.raises(ValueError):
        ops.crop_detections(images, boxes, counts, (8, 8), mean=(0, 0, 0))
    with pytest.raises(YmiError):
        ops.crop_detections([im.cpu() for im in images], boxes, counts, (8, 8))
    with pytest.raises(YmiError):
        ops.crop_detections(images[:-1], boxes, counts, (8, 8))


# ---- graph capture -------------------------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay_with_changed_counts(dev):
    """the op allocates nothing the graph does not own and synchronises nothing: it is captured once and replayed after the counts (and a box) changed in place"""
    from yolort_amd import ops
    case = T.ragged((16, 12), out_dt="f16")
    images = [im.to(dev) for im in case.images]
    boxes, counts = torch.from_numpy(case.boxes).to(dev), torch.tensor(case.counts, dtype=torch.int32, device=dev)
    call = lambda: ops.crop_detections(images, boxes, counts, case.size, dtype=torch.float16)
    call()                                                       # loads the library and the code object outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        crops, index, total = call()
    for new_counts in ([0, 3, 0, 4, 2, 0], [4, 0, 1, 0, 0, 2], [1, 1, 1, 1, 1, 1]):
        other = T.Case("replay", T.RAGGED_SIZES, new_counts, case.size, out_dt="f16", seed=sum(new_counts))
        other.images = case.images
        boxes.copy_(torch.from_numpy(other.boxes))
        counts.copy_(torch.tensor(new_counts, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        w = int(total[0])
        assert total.tolist() == [other.total, 0]
        e_crops, e_index, e_total = call()
        torch.cuda.synchronize()
        assert torch.equal(crops[:w], e_crops[:w]) and torch.equal(index[:w], e_index[:w]) and torch.equal(total, e_total)
        assert torch.equal(index[:w].long().cpu(), other.expected_index())


# ---- the model -----------------------------------------------------------------------------------------------------------------------------------------------------
def _model(dev, thr):
    from workloads.synth import conditioned_weights
    from yolort_amd.models import YOLOv5
    m = YOLOv5(arch=ARCH, size=CANVAS, score_thresh=thr)
    m.load_state_dict(conditioned_weights(m.state_dict(), ARCH, SEED))
    return m.to(dev).half().eval()


def test_model_crop_equals_the_op_on_its_own_detections(dev):
    from workloads.synth import synth_images
    from yolort_amd import ops
    images = [im for im in synth_images(3, *CANVAS, seed=9).to(dev).half()]
    for thr in (0.2, 0.15, 0.1, 0.08):   # (the conditioned recipe places its scores just under 0.26, tests/test_tta_gpu.py)
        m = _model(dev, thr)
        dets = m(images)
        if all(len(d["scores"]) >= 3 for d in dets):
            break
    else:
        pytest.fail("no threshold of the list gives every image three detections")
    lens = [len(d["scores"]) for d in dets]
    print("score_thresh", thr, "detections", lens)
    k = max(lens)
    slab = torch.zeros(len(images), k, 4, device=dev)
    for i, d in enumerate(dets):
        slab[i, : lens[i]] = d["boxes"].float()
    counts = torch.tensor(lens, dtype=torch.int32, device=dev)
    for kw in (dict(), dict(size=(16, 12), square=True, gain=1.3, pad=30, dtype=torch.float32, mean=T.IMAGENET[0], std=T.IMAGENET[1])):
        size = kw.pop("size", (224, 224))
        got = m.crop(images, dets, size=size, **kw)
        want, index, total = ops.crop_detections(images, slab, counts, size, **kw)
        assert total.tolist() == [sum(lens), 0] and [len(c) for c in got] == lens
        assert torch.equal(torch.cat(got), want[: sum(lens)])
        assert index[: sum(lens), 0].tolist() == [i for i, c in enumerate(lens) for _ in range(c)]
        assert float(want[: sum(lens)].float().abs().max()) > 0
    auto = m.crop(images, size=(16, 12))                          # without detections: forward runs first
    assert [len(c) for c in auto] == lens and torch.equal(torch.cat(auto), torch.cat(m.crop(images, dets, size=(16, 12))))
