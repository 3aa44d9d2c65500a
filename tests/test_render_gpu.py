"""Annotated images (include/yolort_amd.h ymi_render, Python `ops.draw_detections` / `YOLOv5.render`) on the GPU: the cases of tests/test_render.py on the real kernel
(same inputs, same expectations, every image inside a poisoned buffer), the public op bit for bit against the painter, graph capture and replay with a changed slab and
changed image contents, and YOLOv5.render on a model's own detections.  Yardstick and cases: tests/_render_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import _render_cases as T
import test_render as CPU

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


def _run(lib, dev, case):
    return T.check(T.run_render(lib, case, dev), case)


def _images(case, dev):
    """the images of a case as the tensors ops.draw_detections takes"""
    return [T.store(img, case.dt).reshape((h, w, 3) if case.dt == "u8hwc" else (3, h, w)).to(dev) for img, (h, w) in zip(case.inputs, case.sizes)]


def _op(case, dev, images=None, **kw):
    from yolort_amd import ops
    images = _images(case, dev) if images is None else images
    names = None if case.names is None else [nm.decode("latin-1") for nm in case.names]
    return ops.draw_detections(images, torch.from_numpy(case.boxes).to(dev), torch.from_numpy(case.scores).to(dev), torch.from_numpy(case.labels).to(dev),
                               torch.tensor(case.counts, dtype=torch.int32, device=dev), names=names, colors=case.colors.tolist(), line_width=case.lw, font_scale=case.fs,
                               labels_on=case.draw_labels, conf=case.draw_conf, txt_color=case.txt, **kw)


def _same(out, case, want):
    return all(torch.equal(o.cpu().reshape(-1), T.store(w, case.dt)) for o, w in zip(out, want))


@pytest.mark.parametrize("dt", T.DTS)
def test_geometry_sweep_of_66_images(dev, lib, dt):
    _run(lib, dev, T.geometry_sweep(dt))


def test_pil_rectangles_agree_with_the_kernel(dev, lib):
    """the eight batches of the CPU file (each asserts that at least 25 of its cases take part: 200 in all)"""
    assert sum(CPU._pil_batch(lib, b, dev) for b in range(T.PIL_BATCHES)) >= 200


@pytest.mark.parametrize("dt", T.DTS)
@pytest.mark.parametrize("offset", [0, 1])
def test_tile_edges_widths_and_misaligned_views(dev, lib, dt, offset):
    _run(lib, dev, T.tiles_case(dt, offset))


def test_only_one_tile_of_one_image_is_touched(dev, lib):
    _run(lib, dev, T.one_tile_case())


@pytest.mark.parametrize("dt", ["u8hwc", "f16"])
def test_lowest_slot_wins(dev, lib, dt):
    _run(lib, dev, T.order_case(dt))


@pytest.mark.parametrize("dt", ["u8hwc", "f32"])
def test_full_slab_of_1024_boxes_on_one_tile(dev, lib, dt):
    _run(lib, dev, T.full_slab_case(dt))


@pytest.mark.parametrize("fs", [1, 2, 3])
@pytest.mark.parametrize("dt", ["u8hwc", "bf16"])
def test_label_placement_names_and_scales(dev, lib, fs, dt):
    _run(lib, dev, T.label_case(fs, dt))


@pytest.mark.parametrize("kw", [dict(draw_conf=False), dict(draw_labels=False)], ids=lambda kw: "-".join(kw))
def test_labels_without_score_and_without_labels(dev, lib, kw):
    _run(lib, dev, T.label_case(2, "u8", **kw))


def test_class_index_labels_without_a_name_table(dev, lib):
    _run(lib, dev, T.index_label_case())


@pytest.mark.parametrize("dt", ["u8hwc", "f16"])
def test_520_scores_print_as_python_formats_them(dev, lib, dt):
    _run(lib, dev, T.scores_case(dt))


@pytest.mark.parametrize("counts", [[0, 4, 0, 3], [4, 4, 4, 4], [3, 5, 1 << 30, 2], [3, -1, 2, -5], [-1, 9, 0, 1]], ids=["zero", "full", "above-k", "negative", "both"])
def test_counts_and_status(dev, lib, counts):
    _run(lib, dev, T.counts_case(counts))


def test_bad_labels_are_skipped_and_reported(dev, lib):
    _run(lib, dev, T.counts_case([4, 4, 4, 4], bad_label=True))
    _run(lib, dev, T.counts_case([4, 0, 0, 4], bad_label=True))


# ---- the public op ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", T.DTS)
def test_op_equals_the_painter_and_leaves_its_inputs_alone(dev, dt):
    for case in (T.label_case(2, dt), T.order_case(dt)):
        want, want_status = case.expected()
        images = _images(case, dev)
        out, status = _op(case, dev, images)
        assert status.is_cuda and status.dtype == torch.int32 and status.tolist() == [want_status]
        assert _same(out, case, want) and _same(images, case, case.inputs), "inplace=False draws on clones"
        same, _ = _op(case, dev, images, inplace=True)
        assert all(a is b for a, b in zip(same, images)) and _same(images, case, want), "inplace=True draws on the inputs themselves"


def test_op_defaults_follow_the_reference(dev):
    """no line width, font scale, colours or names: render_defaults per image, DEFAULT_COLORS, the class index"""
    from yolort_amd import ops
    sizes = [(480, 640), (120, 90)]
    dets = [[T.det(20, 60, 200, 180, 0.9, 3), T.det(100, 100, 400, 250, 0.8, 23)], [T.det(5, 40, 60, 100, 0.7, 1)]]
    lw, fs = zip(*[ops.render_defaults(h, w) for h, w in sizes])
    assert lw == (2, 2) and fs == (2, 1)
    case = T.Case("defaults", "u8hwc", sizes, dets, lw=list(lw), fs=list(fs), names=None, colors=np.array(ops.DEFAULT_COLORS, np.uint8), txt=(255, 255, 255), num_classes=2 ** 31 - 1,
                  claims=(T.OUTLINE, T.BACKGROUND, T.GLYPH))
    out, status = ops.draw_detections(_images(case, dev), torch.from_numpy(case.boxes).to(dev), torch.from_numpy(case.scores).to(dev), torch.from_numpy(case.labels).to(dev),
                                      torch.tensor(case.counts, dtype=torch.int32, device=dev))
    assert status.tolist() == [0] and _same(out, case, case.expected()[0])


def test_refusals(dev, lib):
    from yolort_amd import ops
    from yolort_amd._lib import YmiError
    T.check_refusals(lib, dev)
    case = T.counts_case([3, 3, 3, 3], "f32")
    images = _images(case, dev)
    with pytest.raises(YmiError):
        _op(case, dev, [im.cpu() for im in images])
    with pytest.raises(YmiError):
        _op(case, dev, images[:2] + [im.half() for im in images[2:]])          # mixed dtypes
    with pytest.raises(YmiError):
        _op(case, dev, images[:-1])
    with pytest.raises(YmiError):
        ops.draw_detections(images, torch.zeros(4, T.MAX_K + 1, 4, device=dev), torch.zeros(4, T.MAX_K + 1, device=dev), torch.zeros(4, T.MAX_K + 1, dtype=torch.int64, device=dev),
                            torch.zeros(4, dtype=torch.int32, device=dev))
    for kw in (dict(line_width=0), dict(font_scale=0), dict(colors=[]), dict(txt_color=(0, 300, 0))):
        with pytest.raises(YmiError):
            ops.draw_detections(images, torch.from_numpy(case.boxes).to(dev), torch.from_numpy(case.scores).to(dev), torch.from_numpy(case.labels).to(dev),
                                torch.tensor(case.counts, dtype=torch.int32, device=dev), **kw)
    with pytest.raises(YmiError):
        _op(case, dev, [im.transpose(1, 2) for im in images], inplace=True)    # not contiguous
    torch.cuda.synchronize()
    assert _same(images, case, case.inputs), "a refused call drew nothing"


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay_with_a_changed_slab_and_changed_images(dev, lib):
    """ymi_render allocates nothing and synchronises nothing: captured once on fixed buffers, replayed after the slab AND the image contents changed in place"""
    first, second = T.counts_case([4, 2, 0, 3], "f16"), T.counts_case([1, 4, 3, 0], "f16")
    second.inputs = [np.random.default_rng(77 + i).integers(0, 256, img.shape, dtype=np.uint8) for i, img in enumerate(first.inputs)]
    second.boxes[:, :, 0] += 9
    second.scores[:] = 0.25
    second._expected = None
    bufs, t = T.buffers(first, dev)
    keep = []
    d = T.describe(first, [b.data_ptr() + T.GUARD * b.element_size() for b in bufs], t, keep)
    lib.ymi_render.restype = C.c_int
    warm_bufs, warm_t = T.buffers(first, dev)
    warm = T.describe(first, [b.data_ptr() + T.GUARD * b.element_size() for b in warm_bufs], warm_t, keep)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        assert lib.ymi_render(C.byref(warm), C.c_void_p(stream.cuda_stream)) == 0      # loads the code object outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        assert lib.ymi_render(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(b.cpu()[T.GUARD:-T.GUARD], T.store(img, "f16")) for b, img in zip(bufs, first.inputs)), "capturing draws nothing"
    for case in (first, second):
        for b, img in zip(bufs, case.inputs):
            b[T.GUARD:-T.GUARD] = T.store(img, "f16").to(dev)
        t["boxes"].copy_(torch.from_numpy(case.boxes))
        t["scores"].copy_(torch.from_numpy(case.scores))
        t["counts"].copy_(torch.tensor(case.counts, dtype=torch.int32))
        t["status"][1] = 0
        graph.replay()
        torch.cuda.synchronize()
        T.check(([b.cpu() for b in bufs], t["status"].cpu().tolist()), case)
    assert not np.array_equal(first.expected()[0][0], second.expected()[0][0])


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------------------------
def _model(dev, thr):
    from workloads.synth import conditioned_weights
    from yolort_amd.models import YOLOv5
    m = YOLOv5(arch=ARCH, size=CANVAS, score_thresh=thr)
    m.load_state_dict(conditioned_weights(m.state_dict(), ARCH, SEED))
    return m.to(dev).half().eval()


def test_model_render_equals_the_op_on_its_own_detections(dev):
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
    k = max(lens)
    boxes, scores, labels = torch.zeros(3, k, 4, device=dev), torch.zeros(3, k, device=dev), torch.zeros(3, k, dtype=torch.int64, device=dev)
    for i, d in enumerate(dets):
        boxes[i, : lens[i]], scores[i, : lens[i]], labels[i, : lens[i]] = d["boxes"].float(), d["scores"].float(), d["labels"]
    counts = torch.tensor(lens, dtype=torch.int32, device=dev)
    names = [f"class{i}" for i in range(80)]
    before = [im.clone() for im in images]
    for kw in (dict(), dict(names=names, font_scale=2, line_width=3, conf=False)):
        got = m.render(images, dets, **kw)
        want, status = ops.draw_detections(images, boxes, scores, labels, counts, **kw)
        assert status.tolist() == [0] and len(got) == 3 and all(torch.equal(g, w) for g, w in zip(got, want))
        assert all(torch.equal(a, b) for a, b in zip(images, before)), "the input list is unchanged"
        assert all(not torch.equal(g, b) for g, b in zip(got, before)), "something was drawn into every image"
    auto = m.render(images, names=names)                          # without detections: forward runs first
    again = m.render(images, dets, names=names)
    assert all(torch.equal(a, b) for a, b in zip(auto, again))
    same = m.render(images, dets, inplace=True)
    assert all(a is b for a, b in zip(same, images)) and all(torch.equal(a, b) for a, b in zip(images, m.render(before, dets)))
