"""Annotated images (include/yolort_amd.h ymi_render, Python `ops.draw_detections` / `YOLOv5.render`) without a GPU: the ABI and the signatures, the NumPy painter
against PIL.ImageDraw.rectangle and against Python's score formatting, the committed glyph table against Pillow's font, and render_kernel with its host routing on the
CPU simulator (tests/hipsim: preproc_pool.hip is a simulator unit, so the unchanged simulator build holds the kernel).  Yardstick and cases: tests/_render_cases.py."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _render_cases as T
from test_hipsim_kernels import sim  # noqa: F401  (the module-scoped fixture that builds the simulator library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. constants, ABI, signatures -----------------------------------------------------------------------------------------------------------------------------------
def test_header_text_abi_version_and_struct_size():
    from yolort_amd import _lib
    header = open(os.path.join(ROOT, "include", "yolort_amd.h")).read()
    for text in ("#define YMI_ABI_VERSION 6", "typedef struct ymi_render_desc {", "int ymi_render(const ymi_render_desc* d, void* stream);", "#define YMI_RENDER_MAX_K 1024",
                 "#define YMI_RENDER_NAME_STRIDE 28", "#define YMI_RENDER_STATUS_BAD_COUNT 1", "#define YMI_RENDER_STATUS_STALE_ROW 2", "#define YMI_RENDER_STATUS_BAD_LABEL 4",
                 "common.py:575-652", "plots.py:98-159", "truncated toward zero", "x < X0 + lw or x > X1 - lw or y < Y0 + lw or y > Y1 - lw", "2 * lw <= min(X1 - X0, Y1 - Y0) + 1",
                 "[X0, ty, X0 + w + 1, ty + h + 1]", "outside = (Y0 - h >= 0)", "LOWEST slot", "NO PARITY WITH THE REFERENCE", "ties to even", "?.??", "colors[label % m]"):
        assert text in header, text
    assert _lib.ABI_VERSION == 6 and _lib.load(require_gpu=False).ymi_abi_version() == 6
    assert (_lib.RENDER_STATUS_BAD_COUNT, _lib.RENDER_STATUS_STALE_ROW, _lib.RENDER_STATUS_BAD_LABEL) == (T.BAD_COUNT, T.STALE_ROW, T.BAD_LABEL) == (1, 2, 4)
    assert (_lib.RENDER_MAX_K, _lib.RENDER_NAME_STRIDE) == (T.MAX_K, T.NAME_STRIDE) == (1024, 28)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "yolort_amd.h"\nint main(){printf("%zu %zu %zu %zu %d %d\\n", sizeof(ymi_render_desc), offsetof(ymi_render_desc, status), '
           'offsetof(ymi_render_desc, txt_color), offsetof(ymi_render_desc, k), YMI_RENDER_MAX_K, YMI_RENDER_NAME_STRIDE);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "s")], capture_output=True, text=True, check=True).stdout.split()]
    R = _lib.RenderDesc
    assert out == [C.sizeof(R), R.status.offset, R.txt_color.offset, R.k.offset, 1024, 28], out
    assert "ymi_render" in _lib.EXPORTED_SYMBOLS and _lib._SIGS["ymi_render"] == (C.c_int, [C.POINTER(R), C.c_void_p])


def test_python_signatures_defaults_and_documents():
    from yolort_amd import ops
    from yolort_amd.models import YOLOv5
    p = inspect.signature(ops.draw_detections).parameters
    assert list(p) == ["images", "boxes", "scores", "labels", "counts", "names", "colors", "line_width", "font_scale", "labels_on", "conf", "txt_color", "inplace"]
    kw = ("names", "colors", "line_width", "font_scale", "labels_on", "conf", "txt_color", "inplace")
    assert [p[k].default for k in kw] == [None, None, None, None, True, True, (255, 255, 255), False] and all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in kw)
    assert "no parity with the reference" in ops.draw_detections.__doc__
    q = inspect.signature(YOLOv5.render).parameters
    assert list(q)[:4] == ["self", "images", "detections", "names"] and q["detections"].default is None and q["names"].default is None
    assert len(ops.DEFAULT_COLORS) == 20 == len(set(ops.DEFAULT_COLORS)) and all(len(c) == 3 and all(0 <= v <= 255 for v in c) for c in ops.DEFAULT_COLORS)
    # the reference's defaults: lw = max(round(sum((h, w, 3)) / 2 * 0.003), 2); font size max(round((h + w) / 2 * 0.035), 12) in units of the 11-pixel cell
    assert ops.render_defaults(480, 640) == (2, 2) and ops.render_defaults(1080, 1920) == (5, 5) and ops.render_defaults(100, 100) == (2, 1) and ops.render_defaults(2160, 3840) == (9, 10)
    table = ops.render_name_table(["person", "", "café"])
    assert table.shape == (3, 28) and table[0, :7].tolist() == [6] + list(b"person") and table[1, 0] == 0 and table[2, :5].tolist() == [4] + list(b"caf?")
    with pytest.raises(ValueError):
        ops.render_name_table(["x" * 28])
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "draw_detections" in text and "YOLOv5.render" in text and "1024" in text and "27" in text and "no parity" in text, doc


def test_host_refusals_of_the_library():
    """argument errors come back as YMI_EINVAL with a message before anything is launched (host buffers: a launch would fault)"""
    from yolort_amd import _lib
    T.check_refusals(_lib.load(require_gpu=False))


# ---- 2. the yardsticks themselves --------------------------------------------------------------------------------------------------------------------------------------
def test_committed_glyph_table_equals_pillows_per_character_masks():
    ImageFont = pytest.importorskip("PIL.ImageFont")
    font = ImageFont.load_default_imagefont()
    for code in range(32, 127):
        mask = font.getmask(chr(code))
        assert mask.size == (6, 11)
        assert np.array_equal(np.array(mask).reshape(11, 6) != 0, T.FONT[code - 32]), chr(code)
    assert T.FONT[0].sum() == 0 and all(T.FONT[c - 32].any() for c in range(33, 127))


def test_score_text_is_pythons_formatting_of_the_fp32_value():
    f = np.float32
    text = lambda s: T.label_text(0, s, [b""], True)
    assert [text(v) for v in (0.125, 0.375, 0.625, 0.875)] == [" 0.12", " 0.38", " 0.62", " 0.88"]          # exact ties go to even
    assert [text(v) for v in (0.0, -0.0, 1.0)] == [" 0.00", " -0.00", " 1.00"]
    assert [text(v) for v in (T.NAN, 1.5, -0.1, T.INF, np.nextafter(f(1), f(2)))] == [" ?.??"] * 5
    hi = np.nextafter(f(0.005), f(2))
    assert float(f(0.005)) < 0.005 < float(hi) and [text(f(0.005)), text(hi)] == [" 0.00", " 0.01"]      # fp32(0.005) lies below 0.005, its upper neighbour above
    lo = np.nextafter(f(0.995), f(-1))
    assert float(lo) < 0.995 < float(f(0.995)) and [text(lo), text(f(0.995))] == [" 0.99", " 1.00"]      # fp32(0.995) lies above 0.995, its lower neighbour below
    vals = T.score_values()
    assert len(vals) >= 512 and len({text(v) for v in vals}) >= 100


# ---- 3. the kernel on the simulator -----------------------------------------------------------------------------------------------------------------------------------
def _run(lib, case, device="cpu"):
    return T.check(T.run_render(lib, case, device), case)


@pytest.mark.parametrize("dt", T.DTS)
def test_geometry_sweep_of_66_images_on_the_simulator(sim, dt):
    case = T.geometry_sweep(dt)
    assert len(case.sizes) == 66 and {1, 40} <= {s for hw in case.sizes for s in hw} and set(case.lw) == set(range(1, 8))
    flat = case.boxes[:, :6].reshape(-1, 4)
    assert np.isnan(flat).any() and np.isinf(flat).any() and (np.abs(flat) == 2.0 ** 30).any() and (flat[:, 2] < flat[:, 0]).any(), "the odd boxes are there"
    before = sim.sim_launches()
    _run(sim, case)
    assert sim.sim_launches() - before == 2, "66 images go as two launches"


def _pil_batch(lib, b, device="cpu"):
    """one batch of the PIL comparison -> how many of its 64 cases took part (at least T.PIL_MIN_PER_BATCH of them must)"""
    pytest.importorskip("PIL")
    case = T.pil_batch(b)
    want = _run(lib, case, device)
    took_part = 0
    for i in range(len(case.sizes)):
        if T.pil_takes_part(case, i):
            took_part += 1
            assert np.array_equal(T.pil_image(case, i), want[i]), (case.name, i, case.dets[i], case.lw[i])
    assert took_part >= T.PIL_MIN_PER_BATCH, took_part
    return took_part


def test_at_least_200_cases_take_part_in_the_pil_comparison():
    assert T.PIL_BATCHES * T.PIL_MIN_PER_BATCH >= 200
    took_part = [sum(T.pil_takes_part(case, i) for i in range(64)) for case in map(T.pil_batch, range(T.PIL_BATCHES))]
    print("PIL cases that take part:", took_part)
    assert min(took_part) >= T.PIL_MIN_PER_BATCH and sum(took_part) >= 200
    lws = {case.lw[i] for case in map(T.pil_batch, range(T.PIL_BATCHES)) for i in range(64) if T.pil_takes_part(case, i)}
    assert lws == set(range(1, 8)), "every outline width takes part"


@pytest.mark.parametrize("b", range(T.PIL_BATCHES))
def test_pil_rectangles_agree_with_the_kernel_on_the_simulator(sim, b):
    _pil_batch(sim, b)


@pytest.mark.parametrize("dt", T.DTS)
@pytest.mark.parametrize("offset", [0, 1])
def test_tile_edges_widths_and_misaligned_views_on_the_simulator(sim, dt, offset):
    _run(sim, T.tiles_case(dt, offset))


def test_only_one_tile_of_one_image_is_touched_on_the_simulator(sim):
    case = T.one_tile_case()
    want = _run(sim, case)
    assert np.array_equal(want[0], case.inputs[0]) and np.array_equal(want[2], case.inputs[2])
    rows, cols = np.nonzero((want[1] != case.inputs[1]).any(-1))
    assert 16 <= rows.min() and rows.max() < 32 and 64 <= cols.min() and cols.max() < 128, "the drawing lies inside tile (1, 1)"


@pytest.mark.parametrize("dt", ["u8hwc", "f16"])
def test_lowest_slot_wins_on_the_simulator(sim, dt):
    case = T.order_case(dt)
    want = _run(sim, case)
    c = [tuple(int(v) for v in case.colors[i]) for i in range(3)]
    # (row, column): slot 0's right edge over slot 1's top edge; slot 1's left edge over slot 2's bottom edge; slot 2's bottom edge alone
    assert tuple(want[0][30, 39]) == c[0] and tuple(want[0][49, 21]) == c[1] and tuple(want[0][49, 30]) == c[2], "three overlapping boxes"
    assert tuple(want[1][30, 12]) == c[0] and tuple(want[2][30, 12]) == c[1], "outline over label background, and the reverse"


def test_full_slab_of_1024_boxes_on_one_tile_on_the_simulator(sim):
    _run(sim, T.full_slab_case())


@pytest.mark.parametrize("fs", [1, 2, 3])
def test_label_placement_names_and_scales_on_the_simulator(sim, fs):
    case = T.label_case(fs)
    want = _run(sim, case)
    th = 11 * fs
    colour = tuple(int(v) for v in case.colors[0])
    assert tuple(want[0][0, 3 + 6 * fs * 8 + 1]) == colour, "Y0 - h == 0: the label starts in row 0"
    assert np.array_equal(want[1][: th - 1], case.inputs[1][: th - 1]) and tuple(want[1][th + 11, 3 + 6 * fs * 8 + 1]) == colour, "Y0 - h == -1: the label is inside the box"


@pytest.mark.parametrize("kw", [dict(draw_conf=False), dict(draw_labels=False), dict(draw_labels=False, draw_conf=False)], ids=lambda kw: "-".join(kw))
def test_labels_without_score_and_without_labels_on_the_simulator(sim, kw):
    _run(sim, T.label_case(2, "u8", **kw))


def test_class_index_labels_without_a_name_table_on_the_simulator(sim):
    _run(sim, T.index_label_case())


def test_520_scores_print_as_python_formats_them_on_the_simulator(sim):
    _run(sim, T.scores_case())


@pytest.mark.parametrize("counts,status", [([0, 4, 0, 3], 0), ([4, 4, 4, 4], 0), ([3, 5, 1 << 30, 2], T.BAD_COUNT), ([3, -1, 2, -5], T.STALE_ROW), ([-1, 9, 0, 1], T.BAD_COUNT | T.STALE_ROW)],
                         ids=["zero", "full", "above-k", "negative", "both"])
def test_counts_and_status_on_the_simulator(sim, counts, status):
    case = T.counts_case(counts)
    assert case.expected()[1] == status
    _run(sim, case)


def test_bad_labels_are_skipped_and_reported_on_the_simulator(sim):
    case = T.counts_case([4, 4, 4, 4], bad_label=True)
    assert case.expected()[1] == T.BAD_LABEL
    _run(sim, case)
    _run(sim, T.counts_case([4, 0, 0, 4], bad_label=True))   # the bad labels lie past the counts: no bit


def test_refusals_on_the_simulator(sim):
    T.check_refusals(sim)
