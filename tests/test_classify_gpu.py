"""Second-stage classification on the GPU (include/yolort_amd.h ymi_classify_head / ymi_second_stage_filter): pool_fc_kernel through ops.classify_head bit for bit on
exact operands and within the derived bound on random ones, for every n_split, between poisoned guard bands; second_stage_filter_kernel against the Python loop, with a
graph replay; DarkNetV6 / DarkNetV4.forward, Classify.forward and YOLOv5.classify against their compositions; the refusals.  Cases: tests/_classify_cases.py.  No simulator twin."""
import numpy as np
import pytest
import torch

import _classify_cases as T

pytestmark = pytest.mark.gpu
GUARD, POISON = 64, 1234.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


def _run_head(dev, case, data, dtype, n_split):
    """ops.classify_head on channel-strided views (the slack channels hold NaN) into guarded outputs -> float64 logits; the guard bands are checked"""
    from yolort_amd import ops
    ms, w1, b1, w2, b2 = data
    views = []
    for m, (_, _, c, cs) in zip(ms, case[2]):
        buf = torch.full(m.shape[:3] + (cs,), float("nan"), device=dev, dtype=dtype)
        buf[..., :c] = torch.from_numpy(m).to(dev)
        views.append(buf[..., :c])
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    n = ms[0].shape[0]
    def _guarded(shape, dt, dev):   # a contiguous tensor inside a poisoned buffer -> (whole buffer, the tensor)  # noqa: E306
        big = torch.full((int(np.prod(shape)) + 2 * GUARD,), POISON, device=dev, dtype=dt)
        return big, big[GUARD:-GUARD].view(shape)
    big_o, out = _guarded((n, (w1 if w2 is None else w2).shape[0]), torch.float32, dev)
    big_h, hid = _guarded((n, w1.shape[0]), dtype, dev) if w2 is not None else (None, None)
    got = ops.classify_head(views, t(w1), t(b1), t(w2), t(b2), dtype=dtype, n_split=n_split, out=out, hidden=hid)
    for big in (big_o, big_h):
        assert big is None or (bool((big[:GUARD] == POISON).all()) and bool((big[-GUARD:] == POISON).all())), "a write outside the output"
    return out.double().cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c[0])
def test_head_exact_operands_bit_for_bit_and_random_ones_within_the_bound(dev, case, dtype):
    if case in T.EXACT:   # for every split: the rule's, one, three
        data = T.exact_case(case)
        for n_split in (0, 1, 3):
            np.testing.assert_array_equal(_run_head(dev, case, data, dtype, n_split), T.head_ref(*data), err_msg=f"n_split {n_split}")
    data = T.general_case(case)
    err, tol = np.abs(_run_head(dev, case, data, dtype, 0) - T.head_ref(*data)), T.bound(*data, dtype)
    print(f"{case[0]} {dtype}: max error {err.max():.3e}, smallest bound {tol.min():.3e}, max error / bound {np.max(err / tol):.3f}")
    assert (err <= tol).all()


@pytest.mark.parametrize("name", T.FILTER_CASES)
def test_filter_equals_the_loop(dev, name):
    """kept rows, zeroed tails, counts, cls2 and status; 66 images go in one launch (the kernel has no images-per-launch limit)"""
    from yolort_amd import ops
    arrays = T.filter_case(name)
    *slab, class_map = [None if a is None else torch.from_numpy(a).to(dev) for a in arrays]
    for got, want in zip(ops.second_stage_filter(*slab, class_map=class_map), T.filter_ref(*arrays)):
        np.testing.assert_array_equal(got.cpu().numpy(), np.asarray(want).reshape(got.shape))


def test_filter_graph_capture_and_replays(dev):
    from yolort_amd import ops
    arrays = T.filter_case("alternating")
    ins = [torch.from_numpy(a).to(dev) for a in arrays[:6]]
    ops.second_stage_filter(*ins)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = ops.second_stage_filter(*ins)
    for name in ("keep_all", "keep_none", "ties_nan_inf"):   # same shapes, other logits and labels, written in place
        other = T.filter_case(name)
        ins[2].copy_(torch.from_numpy(other[2]))
        ins[4].copy_(torch.from_numpy(other[4]))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, T.filter_ref(*other)):
            np.testing.assert_array_equal(got.cpu().numpy(), np.asarray(want).reshape(got.shape))


def _tail_check(got, fmaps, layers, dtype, out_dtype):
    """`got` (n, N) against the float64 tail of the NCHW feature maps `fmaps`, within the bound of the general cases plus the output's rounding"""
    ms = [f.double().permute(0, 2, 3, 1).cpu().numpy() for f in fmaps]
    wb = [a for l in layers for a in (l.weight.detach().to(dtype).double().flatten(1).cpu().numpy(), l.bias.detach().double().cpu().numpy())]
    wb += [None, None] * (2 - len(layers))
    want, tol = T.head_ref(ms, *wb), T.bound(ms, *wb, dtype)
    tol = tol + T.UNIT[out_dtype] * (np.abs(want) + tol)
    assert got.dtype == out_dtype and (np.abs(got.double().cpu().numpy() - want) <= tol).all()


@pytest.mark.parametrize("which,dtype", [("v6", torch.float16), ("v6", torch.bfloat16), ("v4", torch.float16)], ids=str)
def test_darknet_forward_and_the_classify_module_are_the_tail_of_their_maps(dev, which, dtype):
    from yolort_amd.models.darknetv4 import DarkNetV4
    from yolort_amd.models.darknetv6 import DarkNetV6
    torch.manual_seed(3)
    m = (DarkNetV6 if which == "v6" else DarkNetV4)(0.33, 0.25, num_classes=10).to(dev).to(dtype).eval()
    x = torch.rand(3, 3, 64, 64, device=dev).to(dtype)
    with torch.no_grad():
        got, fmap = m(x), m.features(x)
    assert tuple(got.shape) == (3, 10)
    _tail_check(got, [fmap], [m.classifier[0], m.classifier[3]], dtype, dtype)
    from yolort_amd.v5 import Classify   # the one-launch head, on a list of maps
    m = Classify(8 + 24, 5).to(dev).half().eval()
    assert list(m.state_dict()) == ["conv.weight", "conv.bias"]
    xs = [torch.rand(33, 8, 7, 7, device=dev).half(), torch.rand(33, 24, 2, 3, device=dev).half()]
    with torch.no_grad():
        got = m(xs)
    _tail_check(got, xs, [m.conv], torch.float16, torch.float16)


def test_yolov5_classify_equals_its_composition(dev):
    """crop -> classifier in chunks of `batch` -> filter, bit for bit; 9 crops in chunks of 4 span three chunks"""
    from yolort_amd import ops
    from yolort_amd.models import YOLOv5
    from yolort_amd.models.darknetv6 import DarkNetV6
    torch.manual_seed(5)
    det = YOLOv5(arch="yolov5_darknet_pan_n_r60", size=(128, 160)).to(dev).half().eval()
    clf = DarkNetV6(0.33, 0.25, num_classes=10).to(dev).half().eval()
    images = [torch.rand(3, 96, 128, device=dev).half(), torch.rand(3, 80, 72, device=dev).half()]
    g = torch.Generator().manual_seed(6)
    dets = []
    for im, cnt in zip(images, (5, 4)):
        xy = torch.rand(cnt, 2, generator=g) * torch.tensor([im.shape[2] - 40.0, im.shape[1] - 40.0])
        dets.append({"boxes": torch.cat([xy, xy + 8 + 30 * torch.rand(cnt, 2, generator=g)], 1).to(dev), "scores": torch.rand(cnt, generator=g).to(dev),
                     "labels": torch.zeros(cnt, dtype=torch.int64, device=dev)})
    boxes, scores, labels, counts, lens = det._slab(dets, 2, dev, "test")

    def composition(lab):
        crops, _, total = ops.crop_detections(images, boxes, counts, (64, 64), capacity=9, square=True, gain=1.3, pad=30)
        logits = torch.cat([clf(crops[r:r + 4]).float() for r in range(0, 9, 4)])
        return ops.second_stage_filter(boxes, scores, lab, counts, logits, total)

    cls2 = composition(labels)[4]
    flip = (torch.arange(labels.numel(), device=dev).view_as(labels) % 2).to(torch.int64)
    labels = (cls2.to(torch.int64).clamp(min=0) + flip) % 10            # every second detection disagrees with the classifier
    for i, d in enumerate(dets):
        d["labels"] = labels[i, : lens[i]]
    ob, os_, ol, oc, _, status = composition(labels)
    got = det.classify(images, clf, dets, size=(64, 64), batch=4)
    assert int(status) == 0 and 0 < int(oc.sum()) < 9
    for i in range(2):
        k = int(oc[i])
        assert torch.equal(got[i]["boxes"], ob[i, :k]) and torch.equal(got[i]["scores"], os_[i, :k]) and torch.equal(got[i]["labels"], ol[i, :k])


def test_refusals(dev):
    from yolort_amd import ops
    from yolort_amd._lib import YmiError
    from yolort_amd.models.darknetv6 import DarkNetV6
    from yolort_amd.v5 import Classify
    with pytest.raises(NotImplementedError, match="g = 1"):
        Classify(16, 4, g=2)
    m = Classify(40, 4).to(dev).half().eval()
    with pytest.raises(YmiError, match="up to four"):
        m([torch.rand(2, 8, 2, 2, device=dev).half()] * 5)
    net = DarkNetV6(0.33, 0.25, num_classes=10).to(dev).eval()
    net.features.compute_dtype = torch.float32
    with pytest.raises(YmiError, match="parity mode"):
        net(torch.rand(1, 3, 64, 64, device=dev))
    with pytest.raises(YmiError, match="no CPU fallback"):
        ops.second_stage_filter(*[torch.from_numpy(a) for a in T.filter_case("keep_all")[:6]])
