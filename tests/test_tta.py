"""Augmented inference (test-time augmentation; include/yolort_amd.h ymi_scale_view / ymi_post_decode_view, Python `augment=True`) without a GPU: the constants and the
ABI, the host logic (view sizes, plan key, refusals), and the two new kernels with their host routing on the CPU simulator (tests/hipsim: preproc_pool.hip and
postprocess.hip are simulator units, so the unchanged simulator build holds them).  Yardsticks and cases: tests/_tta_cases.py."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import _tta_cases as T
from test_hipsim_kernels import sim  # noqa: F401  (the module-scoped fixture that builds the simulator library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_CAP = 4096


# ---- 1. constants and ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_header_text_abi_version_and_struct_sizes():
    from yolort_amd import _lib
    header = open(os.path.join(ROOT, "include", "yolort_amd.h")).read()
    for text in ("#define YMI_ABI_VERSION 6", "int ymi_scale_view(", "int ymi_post_decode_view(const ymi_post_desc* sink, const ymi_post_view* view, void* stream);",
                 "typedef struct ymi_post_view {", "int ymi_plan_add_scale_view(", "int ymi_plan_add_post_decode_view(", "#define YMI_VIEW_PAD 0.447f",
                 "yolo.py:147-163", "torch_utils.py:288-300", "x1' = W - x2 / scale", "differ in rounding only"):
        assert text in header, text
    assert _lib.ABI_VERSION == 6 and _lib.load(require_gpu=False).ymi_abi_version() == 6
    assert (_lib.TTA_SCALES, _lib.TTA_FLIPS, _lib.VIEW_PAD) == (T.SCALES, T.FLIPS, T.PAD)
    # the three existing descriptors keep the sizes they have in the parent's header (x86-64: 216 / 296 / 192 bytes), the new struct matches its ctypes mirror
    src = '#include <stdio.h>\n#include "yolort_amd.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(ymi_conv_desc), sizeof(ymi_post_desc), sizeof(ymi_c3_desc), sizeof(ymi_post_view));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "s")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:3] == [C.sizeof(_lib.ConvDesc), C.sizeof(_lib.PostDesc), C.sizeof(_lib.C3Desc)] == [PARENT_SIZES[k] for k in ("conv", "post", "c3")], out
    assert out[3] == C.sizeof(_lib.PostView)
    for name in ("ymi_scale_view", "ymi_post_decode_view", "ymi_plan_add_scale_view", "ymi_plan_add_post_decode_view"):
        assert name in _lib.EXPORTED_SYMBOLS


PARENT_SIZES = {"conv": 216, "post": 296, "c3": 192}   # sizeof of the three descriptors as the parent commit's header gives them (gcc, x86-64)


# ---- 6. host logic -----------------------------------------------------------------------------------------------------------------------------------------------
def test_view_sizes_equal_the_restated_scale_img():
    from yolort_amd import _lib
    want = {(640, 640): [((531, 531), (544, 544)), ((428, 428), (448, 448))], (128, 160): [((106, 132), (128, 160)), ((85, 107), (96, 128))]}
    for (h, w), gs in (((640, 640), 32), ((128, 160), 32), ((1280, 736), 32), ((1280, 736), 64), ((64, 96), 32)):
        for i, r in enumerate(T.SCALES[1:]):
            assert _lib.tta_view_size(h, w, r, gs) == T.view_sizes(h, w, r, gs), (h, w, r, gs)
            if (h, w) in want:
                assert _lib.tta_view_size(h, w, r, gs) == want[(h, w)][i]
        assert _lib.tta_view_size(h, w, 1.0, gs) == ((h, w), (h, w))
    assert _lib.tta_view_size(64, 96, 0.83) == ((53, 79), (64, 96)) and _lib.tta_view_size(64, 96, 0.67) == ((42, 64), (64, 96))   # pad bands 11 / 17 and 22 / 32
    for strides in ([8, 16, 32], [8, 16, 32, 64]):
        for hw in ((128, 160) if len(strides) == 3 else (128, 192), (640, 640), (1280, 768)):   # sides that are multiples of the largest stride
            shapes = T.view_shapes(*hw, strides)
            assert _lib.tta_layout(shapes) == T.layout(shapes)
            lay, total = T.layout(shapes)
            # what _clip_augmented cuts (yolo.py:201-207): i = (A0 // g) * 1 anchors off the end of view 0, (A2 // g) * 4^(nl - 1) off the front of the last view
            nl, g = len(strides), sum(4 ** x for x in range(len(strides)))
            a0, a2 = sum(3 * h * w for h, w in shapes[0]), sum(3 * h * w for h, w in shapes[-1])
            assert a0 // g == 3 * shapes[0][-1][0] * shapes[0][-1][1] and (a2 // g) * 4 ** (nl - 1) == 3 * shapes[-1][0][0] * shapes[-1][0][1]
            assert total == a0 - a0 // g + sum(3 * h * w for h, w in shapes[1]) + a2 - (a2 // g) * 4 ** (nl - 1)
            assert [m for m, _ in lay] == [1 << (nl - 1), 0, 1]


def _model(**kw):
    from yolort_amd.models import yolo
    return yolo.yolov5_darknet_pan_n_r60(score_thresh=0.25, **kw)


def test_augment_reaches_the_model_and_the_plan_key():
    import yolort_amd.models as Mo
    from yolort_amd import ops
    from yolort_amd.models import yolo
    plain = _model()
    assert plain.augment is False and plain._post_key() == (0.25, 0.45, 300, True, False)   # the key of a model without it is what it always was
    m = _model(augment=True)
    assert m.augment is True and m._post_key() == plain._post_key() + (("augment", True),)
    m.augment = False
    assert m._post_key() == plain._post_key()
    m.augment, m.post_process.merge = True, True
    assert m._post_key()[-1] == ("augment", True) and m._post_key()[:-1] == (0.25, 0.45, 300, True, False, ("merge", 16))
    assert Mo.YOLOv5(arch="yolov5_darknet_pan_n_r60", augment=True).model.augment is True and Mo.yolov5n(augment=True).model.augment is True
    assert yolo.yolov5_darknet_pan_s6_r60(augment=True).augment is True
    for fn in (yolo.YOLO.__init__, yolo.YOLO.load_from_yolov5):
        assert inspect.signature(fn).parameters["augment"].default is False
    ps = list(inspect.signature(ops.postprocess_logits_tta).parameters)
    assert ps[:4] == ["view_outputs", "scales", "flips", "canvas_hw"] and ps[4:] == list(inspect.signature(ops.postprocess_logits).parameters)[1:]
    assert list(inspect.signature(ops.scale_image).parameters) == ["x", "ratio", "flip", "gs"]


def test_augment_refusals():
    from yolort_amd.models import yolo
    from yolort_amd.models.box_head import PostProcess, YOLOHead
    bb = lambda: yolo.darknet_pan_backbone("darknet_n_r6_0", 0.33, 0.25, version="r6.0")

    class OwnHead(YOLOHead):
        pass

    with pytest.raises(ValueError, match="augment=True needs the package's own head"):
        yolo.YOLO(bb(), 80, post_process=torch.nn.Identity(), augment=True)
    b = bb()
    with pytest.raises(ValueError, match="augment=True needs the package's own head"):
        yolo.YOLO(b, 80, head=OwnHead(b.out_channels, 3, [8, 16, 32], 80), augment=True)
    m = yolo.YOLO(bb(), 80, post_process=torch.nn.Identity())
    m.augment = True                       # the live attribute on a model that cannot be augmented: refused at the next batch, before anything is built
    with pytest.raises(ValueError, match="cannot be augmented"):
        m._entry(1, 128, 160, torch.device("cpu"))
    m = _model(augment=True)
    m._augment_check(128, 160)
    for h, w in ((120, 160), (128, 168), (100, 100)):
        with pytest.raises(ValueError, match="multiples of the largest stride 32"):
            m._augment_check(h, w)
        with pytest.raises(ValueError, match="multiples of the largest stride 32"):
            m._entry(1, h, w, torch.device("cpu"))
    p6 = yolo.yolov5_darknet_pan_n6_r60(augment=True)
    p6._augment_check(128, 192)
    with pytest.raises(ValueError, match="largest stride 64"):
        p6._augment_check(128, 160)


def test_host_validation_of_the_new_entry_points():
    """argument errors come back as YMI_EINVAL with a message; nothing is launched, nothing written"""
    from yolort_amd import _lib
    lib = _lib.load(require_gpu=False)
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    assert lib.ymi_scale_view(p, 1, 8, 8, p + 2048, 8, 8, 9, 4, 0, 0, None) == -1 and b"does not fit" in lib.ymi_last_error()
    assert lib.ymi_scale_view(p, 1, 8, 8, p + 2048, 8, 8, 4, 4, 0, 3, None) == -1 and b"dtype" in lib.ymi_last_error()
    assert lib.ymi_scale_view(None, 1, 8, 8, p, 8, 8, 4, 4, 0, 0, None) == -1
    d, v = _lib.PostDesc(), _lib.PostView()
    for f in ("out_boxes", "out_scores", "out_labels", "out_count", "status", "ws"):
        setattr(d, f, p)
    d.num_levels, d.n, d.num_classes, d.detections_per_img, d.cand_cap, d.ws_bytes = 1, 1, 2, 10, 64, 1 << 30
    d.lh[0], d.lw[0] = 1, 4                                   # a sink of 12 anchors
    v.num_levels, v.scale, v.lh[0], v.lw[0], v.lcstride[0] = 1, 0.83, 2, 2, 24
    v.logits[0] = p
    assert lib.ymi_post_decode_view(C.byref(d), None, None) == -1
    v.anchor_base = 1                                         # 12 anchors from index 1: one past the end
    assert lib.ymi_post_decode_view(C.byref(d), C.byref(v), None) == -1 and b"exceed the sink's 12" in lib.ymi_last_error()
    v.anchor_base, v.scale = 0, 0.0
    assert lib.ymi_post_decode_view(C.byref(d), C.byref(v), None) == -1 and b"scale" in lib.ymi_last_error()
    v.scale, v.skip_mask = 1.0, 2
    assert lib.ymi_post_decode_view(C.byref(d), C.byref(v), None) == -1 and b"skip_mask" in lib.ymi_last_error()
    v.skip_mask, v.lcstride[0] = 0, 20
    assert lib.ymi_post_decode_view(C.byref(d), C.byref(v), None) == -1 and b"lcstride" in lib.ymi_last_error()
    assert bytes(buf) == bytes(4096)


# ---- 2. the scale kernel -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "mirror"])
@pytest.mark.parametrize("case", T.SCALE_CASES, ids=lambda c: f"{c[0]}x{c[1]}@{c[2]}")
def test_scale_kernel_on_the_simulator(sim, case, flip, dt):
    h, w, ratio = case
    x = T.canvas(2, h, w, dt)
    got, ch3, guards = T.run_scale(sim, x, ratio, flip, dt)
    T.check_scale(got, ch3, guards, x, ratio, flip, dt)
    if flip:   # the mirror is not a no-op on these inputs
        assert not torch.equal(got, T.run_scale(sim, x, ratio, False, dt)[0])


# ---- 3. the view decode ------------------------------------------------------------------------------------------------------------------------------------------
STRIDES3, ANCH3 = [8, 16, 32], [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
STRIDES4 = [8, 16, 32, 64]
ANCH4 = [[19, 27, 44, 40, 38, 94], [96, 68, 86, 152, 180, 137], [140, 301, 303, 264, 238, 542], [436, 615, 739, 380, 925, 792]]


def _lattice_view(nc, shapes, n=2, seed=0):
    """a few dozen passing cells per level with palette scores (1, 0.5, 0.25: many exact ties) and, for nc > 1, two passing classes in some anchors"""
    g = np.random.default_rng(seed + nc)
    cells = []
    for l, (h, w) in enumerate(shapes):
        for _ in range(min(24, h * w)):
            img, a, y, x = int(g.integers(n)), int(g.integers(3)), int(g.integers(h)), int(g.integers(w))
            cls = {int(g.integers(nc)): (T.HI, T.MID)[int(g.integers(2))]}
            if nc > 1 and g.integers(2):
                cls[int(g.integers(nc))] = T.MID
            cells.append((l, img, a, y, x, (T.HI, T.MID)[int(g.integers(2))], cls))
    return T.lattice_levels(n, shapes, nc, cells)


@pytest.mark.parametrize("nc", [1, 80])
@pytest.mark.parametrize("mode", ["multi", "best", "filter"])
def test_view_decode_equals_the_transformed_scale1_decode_on_the_simulator(sim, nc, mode):
    _view_decode_case(sim, nc, mode, "cpu")


def _view_decode_case(lib, nc, mode, device):
    """one view at a time, whole pyramid at anchor base 0 (scale 0.83 mirrored, scale 0.67 plain, scale 1): boxes = the library's own scale-1 boxes of the same logits
    transformed in numpy float32, bit for bit; scores, labels and order identical.  Lattice logits (exact ties: the order within a view is the plain decode's) and random ones."""
    import _post_cases
    flags = {"multi": 0, "best": T.POST_BEST_CLASS, "filter": T.POST_CLASS_FILTER}[mode]
    classes = None if mode != "filter" else ((0,) if nc == 1 else (0, 3, 17, 41, 79))
    n, k = 2, 600
    seen = 0
    for heads, thr in ((_lattice_view(nc, [(16, 20), (8, 10), (4, 5)]), 0.2), (_post_cases.post_heads(nc, [(6, 7), (3, 4), (2, 2)], n=n, seed=5), 0.5)):
        plain = T.run_views(lib, [dict(heads=heads)], n, nc, STRIDES3, ANCH3, thr, 1.0, k, n * SIM_CAP, flags, classes, device, plain=True)
        assert int(plain["status"][1]) == 0 and int(plain["count"].max()) < k
        for scale, flip_w in ((0.83, 160), (0.67, 0), (1.0, 0)):
            out = T.run_views(lib, [dict(heads=heads, scale=scale, flip_w=flip_w)], n, nc, STRIDES3, ANCH3, thr, 1.0, k, n * SIM_CAP, flags, classes, device)
            assert torch.equal(out["count"], plain["count"]) and torch.equal(out["scores"], plain["scores"]) and torch.equal(out["labels"], plain["labels"])
            assert torch.equal(out["status"][:5], plain["status"][:5])
            for i in range(n):
                b, _, _ = T.rows(plain, i)
                np.testing.assert_array_equal(T.rows(out, i)[0], T.descale32(b, scale, flip_w))
                seen += len(b)
            assert (out["boxes"][0, int(out["count"][0]):] == T.GUARD).all()
    assert seen > 100
    return seen


ONE_BODY_PARAMS = ((3, 0.3), (171, 0.0))   # (num_classes, score_thresh); 171 classes at a threshold <= 0: 3 * 171 = 513 records per pixel > DEC_BUF = 512, the flush in mid-pixel
ONE_BODY_MODES = {"multi": (0, False), "multi-filter": (0, True), "best": (T.POST_BEST_CLASS, False), "best-filter": (T.POST_BEST_CLASS, True)}
ONE_BODY_CAP = 2 * 16384                   # per image more than the 63 * 171 = 10773 records of the second parameter set


def _one_body_case(lib, nc, thr, mode, device):
    """decode_kernel and decode_view_kernel are two entry points of ONE body: ymi_post_begin, one ymi_post_decode_view with scale 1, no mirror, anchor base 0 and no
    skipped level, ymi_post_finish == ymi_postprocess of the same logits BIT FOR BIT in boxes, scores, labels, counts and all status words (a division by 1.0 is exact).
    Two images over levels of 4 x 4, 2 x 2 and 1 x 1: a wave walks 8 pixels, so in the two coarse levels (8 and 2 pixels in all) the image changes inside a wave."""
    import _post_cases
    flags, filtered = ONE_BODY_MODES[mode]
    classes = None if not filtered else ((0, 2) if nc == 3 else (0, 3, 17, 41, 79, 170))
    flags |= T.POST_CLASS_FILTER if filtered else 0
    n, k = 2, 300
    heads = _post_cases.post_heads(nc, [(4, 4), (2, 2), (1, 1)], n=n, seed=23)
    plain = T.run_views(lib, [dict(heads=heads)], n, nc, STRIDES3, ANCH3, thr, 0.45, k, ONE_BODY_CAP, flags, classes, device, plain=True)
    view = T.run_views(lib, [dict(heads=heads, scale=1.0, flip_w=0, base=0, skip=0)], n, nc, STRIDES3, ANCH3, thr, 0.45, k, ONE_BODY_CAP, flags, classes, device)
    print(f"nc {nc} thr {thr} {mode}: status {plain['status'].tolist()} counts {plain['count'].tolist()}")
    assert int(plain["status"][1]) == 0 and int(plain["count"].min()) > 0
    if nc == 171 and mode == "multi":
        assert int(plain["status"][4]) == n * 63 * 171   # every (anchor, class) pair of every pixel: 513 records per pixel
    for key in ("boxes", "scores", "labels", "count", "status"):
        assert torch.equal(view[key], plain[key]), key
    return plain


@pytest.mark.parametrize("mode", list(ONE_BODY_MODES))
@pytest.mark.parametrize("nc,thr", ONE_BODY_PARAMS)
def test_scale1_view_decode_equals_the_plain_decode_bit_for_bit_on_the_simulator(sim, nc, thr, mode):
    _one_body_case(sim, nc, thr, mode, "cpu")


def _union_case(lib, nc, flags, classes, device, strides=STRIDES3, anchors=ANCH3, hw=T.CANVAS):
    """three views with their tails clipped, nms_thresh 1.0: every candidate comes out, in the order of torch.cat(y, 1) under a stable sort by score"""
    shapes = T.view_shapes(*hw, strides)
    n, k, thr = 2, 900, 0.2
    view_heads = [_lattice_view(nc, sh, n=n, seed=10 * v) for v, sh in enumerate(shapes)]
    views, total = T.tta_views(view_heads, hw[1])
    out = T.run_views(lib, views, n, nc, strides, anchors, thr, 1.0, k, n * SIM_CAP, flags, classes, device)
    want = T.expected_union(lib, view_heads, hw[1], n, nc, strides, anchors, thr, k, n * SIM_CAP, flags, classes, device)
    assert int(out["status"][1]) == 0
    for i, (b, s, lab) in enumerate(want):
        gb, gs, gl = T.rows(out, i)
        assert len(gs) == len(s) > 20, (len(gs), len(s))
        np.testing.assert_array_equal(gs, s), np.testing.assert_array_equal(gl, lab), np.testing.assert_array_equal(gb, b)
    return out


@pytest.mark.parametrize("flags,classes", [(0, None), (T.POST_BEST_CLASS, None), (T.POST_CLASS_FILTER, (1,))], ids=["multi", "best", "filter"])
def test_three_views_anchor_bases_and_tie_order_on_the_simulator(sim, flags, classes):
    _union_case(sim, 2, flags, classes, "cpu")


def _tie_and_tail_case(lib, device, strides, anchors, hw):
    """ties across views: the same score in view 0 and view 1, far apart -> view 0 first; tails: a hot cell only in the coarsest level of view 0 and only in the finest of the
    last view yields nothing, the same cells in kept levels yield one detection each"""
    shapes = T.view_shapes(*hw, strides)
    nl, nc, n = len(strides), 2, 1
    hot = lambda l, y, x: (l, 0, 0, y, x, T.HI, {1: T.HI})
    empty = lambda v: T.lattice_levels(n, shapes[v], nc, [])
    run = lambda vh: T.run_views(lib, T.tta_views(vh, hw[1])[0], n, nc, strides, anchors, 0.5, 0.45, 10, SIM_CAP, 0, None, device)
    # tails
    out = run([T.lattice_levels(n, shapes[0], nc, [hot(nl - 1, 0, 0)]), empty(1), T.lattice_levels(n, shapes[2], nc, [hot(0, 1, 1)])])
    assert int(out["count"][0]) == 0 and int(out["status"][4]) == 0
    out = run([T.lattice_levels(n, shapes[0], nc, [hot(nl - 2, 0, 0)]), empty(1), empty(2)])
    assert int(out["count"][0]) == 1
    out = run([empty(0), empty(1), T.lattice_levels(n, shapes[2], nc, [hot(1, 1, 1)])])
    assert int(out["count"][0]) == 1
    out = run([empty(0), T.lattice_levels(n, shapes[1], nc, [hot(nl - 1, 0, 0), hot(0, 1, 1)]), empty(2)])   # the middle view keeps every level
    assert int(out["count"][0]) == 2
    # ties: view 1's cell sits at a LOWER anchor index within its view than view 0's, and still comes second; boxes far apart (no suppression)
    y0, x0 = shapes[0][0][0] - 1, shapes[0][0][1] - 1
    out = run([T.lattice_levels(n, shapes[0], nc, [hot(0, y0, x0)]), T.lattice_levels(n, shapes[1], nc, [hot(0, 0, shapes[1][0][1] - 1)]), empty(2)])
    assert int(out["count"][0]) == 2 and out["scores"][0, 0] == out["scores"][0, 1] == 1.0
    b = out["boxes"][0, :2].numpy()
    s8 = T.F32(strides[0])
    cx0 = (T.F32(x0) + T.F32(0.5)) * s8                                                      # view 0: centre of its last cell
    cx1 = T.F32(hw[1]) - ((T.F32(shapes[1][0][1] - 1) + T.F32(0.5)) * s8) / T.F32(0.83)      # view 1: mirrored back, its LAST column is the canvas's left edge
    assert abs((b[0, 0] + b[0, 2]) / 2 - cx0) < 1e-3 and abs((b[1, 0] + b[1, 2]) / 2 - cx1) < 1e-3, (b, cx0, cx1)
    assert b[0, 0] > b[1, 2]   # far apart: view 0's box at the right edge, view 1's at the left


# ---- 4. tails (and ties across views) ----------------------------------------------------------------------------------------------------------------------------
def test_tails_and_cross_view_ties_on_the_simulator(sim):
    _tie_and_tail_case(sim, "cpu", STRIDES3, ANCH3, T.CANVAS)


def test_tails_of_a_p6_geometry_on_the_simulator(sim):
    _tie_and_tail_case(sim, "cpu", STRIDES4, ANCH4, (128, 192))


# ---- 5. the whole post-process of three views against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", T.WHOLE_RUNS, ids=lambda r: f"nc{r[0]}-{'best' if r[4] else 'multi'}-{'agnostic' if r[5] else 'aware'}-{'filter' if r[6] else 'all'}-{'merge' if r[7] else 'plain'}")
def test_whole_post_process_of_three_views_vs_the_oracle_on_the_simulator(sim, run):
    _whole_case(sim, run, "cpu")


def _whole_case(lib, run, device):
    nc, thr, nms, k, best, agnostic, classes, merge = run
    view_heads, strides, anchors = T.whole_case(nc)
    n = view_heads[0][0].shape[0]
    xywh, conf = T.oracle_union(view_heads, T.CANVAS[1], strides, anchors)
    ref, cands = T.oracle_reference(xywh, conf, thr, nms, k, best, agnostic, classes, merge)
    counts = [len(s) for _, s, _ in cands]
    print(run, "candidates", counts, "detections", [len(r["scores"]) for r in ref])
    assert min(counts) > 20 and all(0 < len(r["scores"]) < c for r, c in zip(ref, counts))   # the NMS suppresses something in every image
    views, _ = T.tta_views(view_heads, T.CANVAS[1])
    out = T.run_views(lib, views, n, nc, strides, anchors, thr, nms, k, n * SIM_CAP, T.run_flags(best, agnostic, classes, merge), classes, device)
    assert int(out["status"][1]) == 0 and int(out["status"][4]) == sum(counts)
    T.assert_equals_reference(out, ref, str(run))
    return out
