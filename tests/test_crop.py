"""Detection crops (include/yolort_amd.h ymi_crop_resize, Python `ops.crop_detections` / `YOLOv5.crop`) without a GPU: the ABI, the rectangle arithmetic against the
reference's own rectangles (tests/golden/crop_rects.json), and crop_resize_kernel with its host routing on the CPU simulator (tests/hipsim: preproc_pool.hip is a
simulator unit, so the unchanged simulator build holds the kernel).  Yardsticks and cases: tests/_crop_cases.py."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import _crop_cases as T
from test_hipsim_kernels import sim  # noqa: F401  (the module-scoped fixture that builds the simulator library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_SIZES = {"conv": 216, "post": 296, "c3": 192}   # sizeof of the three descriptors as the parent commit's header gives them (gcc, x86-64)


# ---- 1. constants and ABI ------------------------------------------------------------------------------------------------------------------------------------------
def test_header_text_abi_version_and_struct_sizes():
    from yolort_amd import _lib
    header = open(os.path.join(ROOT, "include", "yolort_amd.h")).read()
    for text in ("#define YMI_ABI_VERSION 6", "typedef struct ymi_crop_desc {", "int ymi_crop_resize(const ymi_crop_desc* d, void* stream);",
                 "#define YMI_CROP_STATUS_CAPACITY 1", "#define YMI_CROP_STATUS_BAD_COUNT 2", "plots.py:545-558", "general.py:691-723", "common.py:644",
                 "w = w * gain + pad", "truncated toward zero", "fmaf(scale, dst + 0.5, -0.5)", "fma(w11, v11, fma(w10, v10, fma(w00, v00, fl(w01 * v01))))",
                 "(v - mean[c]) / std[c]", "offset[i] + j", "cv2.resize on uint8 uses fixed-point weights"):
        assert text in header, text
    assert _lib.ABI_VERSION == 6 and _lib.load(require_gpu=False).ymi_abi_version() == 6
    assert (_lib.CROP_STATUS_CAPACITY, _lib.CROP_STATUS_BAD_COUNT) == (T.STATUS_CAPACITY, T.STATUS_BAD_COUNT) == (1, 2)
    src = ('#include <stdio.h>\n#include "yolort_amd.h"\nint main(){printf("%zu %zu %zu %zu %d %d\\n", sizeof(ymi_conv_desc), sizeof(ymi_post_desc), sizeof(ymi_c3_desc), '
           'sizeof(ymi_crop_desc), YMI_CROP_STATUS_CAPACITY, YMI_CROP_STATUS_BAD_COUNT);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "s")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[:3] == [C.sizeof(_lib.ConvDesc), C.sizeof(_lib.PostDesc), C.sizeof(_lib.C3Desc)] == [PARENT_SIZES[k] for k in ("conv", "post", "c3")], out
    assert out[3] == C.sizeof(_lib.CropDesc) and out[4:] == [1, 2], out
    assert "ymi_crop_resize" in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGS["ymi_crop_resize"] == (C.c_int, [C.POINTER(_lib.CropDesc), C.c_void_p])


def test_python_signatures_and_documents():
    from yolort_amd import ops
    from yolort_amd.models import YOLOv5
    p = inspect.signature(ops.crop_detections).parameters
    assert list(p) == ["images", "boxes", "counts", "size", "gain", "pad", "square", "mean", "std", "dtype", "capacity"]
    assert [p[k].default for k in ("gain", "pad", "square", "mean", "std", "dtype", "capacity")] == [1.02, 10, False, None, None, torch.float16, None]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("gain", "pad", "square", "mean", "std", "dtype", "capacity"))
    assert "canvas" in ops.crop_detections.__doc__.lower() and "not claimed as parity" in ops.crop_detections.__doc__
    q = inspect.signature(YOLOv5.crop).parameters
    assert list(q)[:4] == ["self", "images", "detections", "size"] and q["detections"].default is None and q["size"].default == (224, 224)
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "crop_detections" in text and "YOLOv5.crop" in text and "F.interpolate" in text and "cv2" in text, doc


def test_host_refusals_of_the_library():
    """argument errors come back as YMI_EINVAL with a message before anything is launched (host buffers: a launch would fault)"""
    from yolort_amd import _lib
    T.check_refusals(_lib.load(require_gpu=False))


# ---- 2. the rectangle ----------------------------------------------------------------------------------------------------------------------------------------------
def test_golden_file_covers_what_it_should():
    groups = T.golden_groups()
    assert 180 <= sum(len(g["boxes"]) for g in groups) <= 260
    assert {(g["gain"], g["pad"], g["square"]) for g in groups} >= {(1.02, 10, False), (1.3, 30, True), (1.0, 0, False)}
    for g in groups:
        b, r = np.asarray(g["boxes"], np.float64), np.asarray(g["rects"])
        assert (b == b.astype(np.float32)).all(), "boxes are stored as the doubles that equal their fp32 values"
        h, w = g["h"], g["w"]
        assert (b[:, 0] < 0).any() and (b[:, 2] > w).any() and (b[:, 1] < 0).any() and (b[:, 3] > h).any(), "boxes across every edge"
        assert ((b[:, 2] < 0) | (b[:, 0] > w) | (b[:, 3] < 0) | (b[:, 1] > h)).sum() >= 4, "boxes wholly outside"
        assert (((b[:, 2] - b[:, 0]) < 1) & ((b[:, 2] - b[:, 0]) > 0)).any(), "boxes thinner than a pixel"
        assert ((b[:, 3] - b[:, 1]) > 3 * (b[:, 2] - b[:, 0])).any() and ((b[:, 2] - b[:, 0]) > 3 * (b[:, 3] - b[:, 1])).any(), "tall and wide boxes"
        assert (r[:, 0::2] >= 0).all() and (r[:, 0::2] <= w).all() and (r[:, 1::2] >= 0).all() and (r[:, 1::2] <= h).all()
        empty = (r[:, 2] <= r[:, 0]) | (r[:, 3] <= r[:, 1])
        assert empty.any() and (~empty).sum() >= 15


def test_golden_has_corners_within_an_ulp_of_an_integer():
    """after `* gain + pad` a corner of some boxes is an integer >= 1 or its fp32 neighbour on either side: truncation decides on the last bit.  Every group has several
    such corners, and over the file at least five are a neighbour (not the integer itself)"""
    neighbours = 0
    for g in T.golden_groups():
        b = torch.tensor(g["boxes"], dtype=torch.float32)
        gain, pad, two = (torch.tensor(v, dtype=torch.float32) for v in (g["gain"], g["pad"], 2.0))
        bw, bh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        if g["square"]:
            bw = bh = torch.maximum(bw, bh)
        left = ((b[:, 0] + b[:, 2]) / two - (bw * gain + pad) / two).numpy()
        top = ((b[:, 1] + b[:, 3]) / two - (bh * gain + pad) / two).numpy()
        near = 0
        for c in np.concatenate([left, top]):
            t = np.float32(np.round(c))
            beside = t >= 1 and c in (np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf)))
            near += int(beside or (t >= 1 and c == t))
            neighbours += int(beside)
        assert near >= 4, (g["h"], g["w"], near)
    assert neighbours >= 5, neighbours


def test_restated_rectangle_equals_the_reference_rectangles():
    for g in T.golden_groups():
        assert torch.equal(T.rect_ref(g["boxes"], g["h"], g["w"], g["gain"], g["pad"], g["square"]), torch.tensor(g["rects"])), (g["h"], g["w"], g["gain"])


@pytest.mark.parametrize("gi", range(5))
def test_library_rectangles_equal_the_reference_rectangles_on_the_simulator(sim, gi):
    _golden_case(sim, gi, "cpu")


def _golden_case(lib, gi, device):
    """the index rows of the library for the golden boxes == the reference's rectangles as the reference leaves them, empty ones (with their clipped corners) included,
    and the crops are right too (all zero for the empty ones)"""
    g = T.golden_groups()[gi]
    case = T.golden_case(g)
    out = T.run_crop(lib, case, device)
    want = torch.tensor(g["rects"])
    assert torch.equal(out["index"][: case.total, 2:].long(), want)
    empty = [i for i, r in enumerate(want.tolist()) if T.is_empty(r)]
    assert len(empty) >= 4 and any(want[i].any() for i in empty), "empty golden rectangles, some with corners other than zero"
    assert all(bool((out["crops"][i] == 0).all()) for i in empty)
    T.check_crop(out, case)
    return out


# ---- 3. pixels -----------------------------------------------------------------------------------------------------------------------------------------------------
EXACT = [(size, "f32", out_dt) for size in T.SIZES for out_dt in T.OUT_DTS] + [(size, "u8hwc", "f32") for size in T.SIZES] + [((8, 8), "u8", "f16"), ((16, 12), "bf16", "bf16"),
                                                                                                                               ((7, 5), "f16", "f16")]


@pytest.mark.parametrize("size,in_dt,out_dt", EXACT, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_power_of_two_weights_are_bit_exact_on_the_simulator(sim, size, in_dt, out_dt):
    _run(sim, T.exact_case(size, in_dt, out_dt), "cpu")


def test_normalised_identity_is_bit_exact_on_the_simulator(sim):
    _run(sim, T.exact_case((8, 8), "u8hwc", "f32", *T.IMAGENET), "cpu")


def _run(lib, case, device):
    out = T.run_crop(lib, case, device)
    T.check_crop(out, case)
    return out


@pytest.mark.parametrize("out_dt", T.OUT_DTS)
def test_up_and_down_scaling_on_the_simulator(sim, out_dt):
    out = _run(sim, T.scaling_case(out_dt), "cpu")
    assert out["index"][:4, 2:].tolist() == [[10, 5, 12, 8], [20, 30, 21, 31], [1, 2, 62, 45], [0, 0, 64, 48]]
    one = out["crops"][1]
    assert float((one - one[:, :1, :1]).abs().max()) <= T.pixel_tolerance(out_dt)   # a 1 x 1 rectangle: every output pixel is that pixel (up to the roundings of its four weights)


@pytest.mark.parametrize("size", T.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("params", [dict(), dict(square=True, gain=1.3, pad=30), dict(mean=T.IMAGENET[0], std=T.IMAGENET[1]), dict(out_dt="f16", mean=T.IMAGENET[0], std=T.IMAGENET[1])],
                         ids=["save_one_box", "apply_classifier", "normalised", "normalised-f16"])
def test_ragged_counts_on_the_simulator(sim, size, params):
    case = T.ragged(size, **params)
    out = _run(sim, case, "cpu")
    assert out["index"][: case.total, 0].tolist() == [1, 1, 1, 3, 3, 3, 3, 4, 4] and out["index"][: case.total, 1].tolist() == [0, 1, 2, 0, 1, 2, 3, 0, 1]


@pytest.mark.parametrize("in_dt", T.IN_DTS)
@pytest.mark.parametrize("out_dt", T.OUT_DTS)
def test_every_input_and_output_dtype_on_the_simulator(sim, in_dt, out_dt):
    _run(sim, T.ragged((8, 8), in_dt=in_dt, out_dt=out_dt), "cpu")


# ---- 4. layout and bookkeeping -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(8, 8), (7, 5)], ids=["wide", "scalar"])
def test_66_images_cross_the_launch_boundary_with_global_offsets_on_the_simulator(sim, size):
    case = T.many_images_case(size)
    assert len(case.sizes) == 66 and case.clamped[0] == 0 and case.clamped[33] == 0 and case.clamped[65] == 3 and case.clamped[64] > 0
    before = sim.sim_launches()
    out = _run(sim, case, "cpu")
    assert sim.sim_launches() - before == 2
    assert out["index"][case.total - 3: case.total, 0].tolist() == [65, 65, 65]


def _capacity_cases(lib, device):
    full = T.ragged((8, 8))
    ref = T.run_crop(lib, full, device)
    T.check_crop(ref, full)
    for cap in (full.total, full.total - 1, 0):
        case = T.ragged((8, 8), cap=cap)
        out = T.run_crop(lib, case, device)
        T.check_crop(out, case)
        assert out["total"].tolist() == [cap, T.STATUS_CAPACITY if cap < full.total else 0]
        assert torch.equal(out["crops"][:cap], ref["crops"][:cap]) and torch.equal(out["index"][:cap], ref["index"][:cap]), "the first rows are intact"


def test_capacity_equal_below_and_zero_on_the_simulator(sim):
    _capacity_cases(sim, "cpu")


def _bad_count_cases(lib, device):
    for counts, clamped in (([0, 3, 0, 5, 2, 0], [0, 3, 0, 4, 2, 0]), ([0, 3, -1, 4, 2, 0], [0, 3, 0, 4, 2, 0]), ([2, 3, 0, 4, 2, 1 << 30], [2, 3, 0, 4, 2, 4])):
        case = T.Case(f"counts-{counts}", T.RAGGED_SIZES, counts, (8, 8), cap=20)
        assert case.clamped == clamped and case.expected_status() == T.STATUS_BAD_COUNT
        out = T.run_crop(lib, case, device)
        T.check_crop(out, case)
        assert out["total"].tolist() == [sum(clamped), T.STATUS_BAD_COUNT]


def test_count_above_k_or_negative_sets_the_status_bit_on_the_simulator(sim):
    _bad_count_cases(sim, "cpu")


def test_non_finite_boxes_give_zero_crops_on_the_simulator(sim):
    out = _run(sim, T.nonfinite_case(), "cpu")
    rects = out["index"][:8, 2:].tolist()
    assert [r == [0, 0, 0, 0] for r in rects] == [True, True, True, False, True, True, False, True], rects
    assert all(bool((out["crops"][i] == 0).all()) == (rects[i] == [0, 0, 0, 0]) for i in range(8))


def test_empty_batch_and_empty_slab_on_the_simulator(sim):
    for case in (T.Case("no-images", [], [], (8, 8), cap=3), T.Case("no-detections", [(8, 8), (8, 8)], [0, 0], (8, 8), cap=3)):
        out = _run(sim, case, "cpu")
        assert out["total"].tolist() == [0, 0]


def test_refusals_on_the_simulator(sim):
    T.check_refusals(sim)
