"""Merge-NMS (include/yolort_amd.h YMI_POST_MERGE / YMI_POST_MERGE_KEEP_SINGLE; Python `merge=True`, `merge_redundant=`) without a GPU: the constants and the Python
surface, the refusals, the plan key, the yardstick of tests/_merge_cases.py on a hand-made case, the non-vacuity of every case from the yardstick alone, and
merge_gather_kernel with its host routing on the CPU simulator (tests/hipsim: postprocess.hip is a simulator unit, so the unchanged simulator build holds the new kernel),
through ymi_postprocess with a dirty workspace and pre-filled outputs.  Every test of this file passes under both lane orders (HIPSIM_REVERSE=1)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import _agnostic_cases as A
import _merge_cases as M
from test_best_class import _nhwc_logits, _post_desc
from test_hipsim_kernels import _check, sim  # noqa: F401  (sim: the module-scoped fixture that builds the simulator library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -3.0


# ---- host logic ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_constants_header_text_and_abi_version():
    from yolort_amd import _lib
    assert _lib.POST_MERGE == 16 == M.POST_MERGE and _lib.POST_MERGE_KEEP_SINGLE == 32 == M.POST_MERGE_KEEP_SINGLE
    assert (_lib.POST_EXACT_FULL, _lib.POST_BEST_CLASS, _lib.POST_AGNOSTIC, _lib.POST_CLASS_FILTER) == (1, 2, 4, 8)
    assert _lib.merge_flags(False, False) == 0 and _lib.merge_flags(True) == 16 and _lib.merge_flags(True, False) == 48
    header = open(os.path.join(ROOT, "include", "yolort_amd.h")).read()
    for text in ("#define YMI_POST_MERGE 16", "#define YMI_POST_MERGE_KEEP_SINGLE 32", "#define YMI_MERGE_MAX_N 3000", "#define YMI_ABI_VERSION 6",
                 "general.py:604-613", "4096 x class", "no max_nms cut", "where the reference would emit NaN"):
        assert text in header, text
    assert _lib.load(require_gpu=False).ymi_abi_version() == 6   # two new flag values, no struct change: a caller built against the previous header keeps working


def test_keep_single_without_merge_is_refused():
    """host validation comes first: YMI_EINVAL by name, nothing launched, nothing written"""
    from yolort_amd import _lib
    lib = _lib.load(require_gpu=False)
    d = _lib.PostDesc()
    buf = (C.c_char * 64)()
    for f in ("out_boxes", "out_scores", "out_labels", "out_count", "status", "ws"):
        setattr(d, f, C.addressof(buf))
    d.num_levels, d.n, d.num_classes, d.detections_per_img, d.cand_cap, d.ws_bytes = 1, 1, 2, 10, 64, 64
    d.lh[0], d.lw[0] = 2, 2
    d.flags = M.POST_MERGE_KEEP_SINGLE
    for call in (lib.ymi_postprocess, lib.ymi_post_begin, lib.ymi_post_finish):
        assert call(C.byref(d), None) == -1 and b"YMI_POST_MERGE_KEEP_SINGLE without YMI_POST_MERGE" in lib.ymi_last_error()
    assert bytes(buf) == bytes(64)


def test_merge_kwargs_reach_the_post_process():
    import yolort_amd.models as Mo
    from yolort_amd import ops
    from yolort_amd.models import yolo
    from yolort_amd.models.box_head import PostProcess
    pp = PostProcess([8, 16, 32], 0.25, 0.45, 300)
    assert pp.merge is False and pp.merge_redundant is True
    assert list(inspect.signature(PostProcess.__init__).parameters)[-1] == "agnostic"   # the parameter list is the one it was: attributes, like `classes`
    makers = [lambda **kw: yolo.yolov5_darknet_pan_n_r60(**kw), lambda **kw: Mo.YOLOv5(arch="yolov5_darknet_pan_n_r60", **kw).model, lambda **kw: Mo.yolov5n(**kw).model,
              lambda **kw: yolo.YOLO(yolo.darknet_pan_backbone("darknet_n_r6_0", 0.33, 0.25, version="r6.0"), 80, **kw)]
    for make in makers:
        m = make()
        assert m.post_process.merge is False and m.post_process.merge_redundant is True
        m = make(merge=True, agnostic=True, score_thresh=0.3)
        assert m.post_process.merge is True and m.post_process.merge_redundant is True and m.post_process.agnostic is True and m.post_process.score_thresh == 0.3
        m = make(merge=True, merge_redundant=False, classes=[0, 2])
        assert m.post_process.merge is True and m.post_process.merge_redundant is False and m.post_process.classes == (0, 2)
    factories = [n for n in dir(yolo) if n.startswith("yolov5_") and callable(getattr(yolo, n))]
    assert len(factories) >= 16, factories
    for name in factories[:16] if len(factories) == 16 else factories:
        sig = inspect.signature(getattr(yolo, name))
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in sig.parameters.values()), name   # **kwargs -> YOLO(...)
    for fn in (yolo.YOLO.__init__, yolo.YOLO.load_from_yolov5, ops.postprocess_logits):
        ps = inspect.signature(fn).parameters
        assert ps["merge"].default is False and ps["merge_redundant"].default is True, fn


def test_merge_next_to_an_injected_post_process_is_refused():
    from yolort_amd.models import yolo
    from yolort_amd.models.box_head import PostProcess
    bb = lambda: yolo.darknet_pan_backbone("darknet_n_r6_0", 0.33, 0.25, version="r6.0")
    own = PostProcess([8, 16, 32], 0.25, 0.45, 300)
    with pytest.raises(ValueError, match="merge"):
        yolo.YOLO(bb(), 80, post_process=own, merge=True)
    with pytest.raises(ValueError, match="merge"):
        yolo.YOLO(bb(), 80, post_process=own, merge_redundant=False)
    own.merge = True   # the way to configure an injected module
    assert yolo.YOLO(bb(), 80, post_process=own).post_process.merge is True


def test_the_plan_key_of_merge():
    """a model without merge keeps exactly the key it has; with merge a further element that tells the two merge_redundant values apart and is not the filter's True"""
    from yolort_amd.models import yolo
    m = yolo.yolov5_darknet_pan_n_r60(score_thresh=0.25)
    plain = m._post_key()
    assert plain == (0.25, 0.45, 300, True, False)
    m.post_process.merge_redundant = False          # without merge the attribute means nothing: the same plan
    assert m._post_key() == plain
    m.post_process.merge = True
    k_single = m._post_key()
    m.post_process.merge_redundant = True
    k_merge = m._post_key()
    assert len({plain, k_single, k_merge}) == 3 and k_merge[:5] == plain and k_single[:5] == plain and len(k_merge) == 6
    m.post_process.classes = [1]
    k_both = m._post_key()
    assert k_both[:6] == plain + (True,) and len(k_both) == 7 and k_both[6] == k_merge[5] and k_both[6] is not True
    m.post_process.merge = False
    assert m._post_key() == plain + (True,)         # the filter form, as it was
    m.post_process.classes = None
    assert m._post_key() == plain
    assert k_merge != plain + (True,) and k_single != plain + (True,)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------------------------------------
def _hand_made():
    b = np.array([[0, 0, 8, 8], [2, 0, 10, 8], [100, 100, 108, 108]], np.float32)
    return [(b[[0, 2, 1]], np.array([0.5, 0.5, 0.25], np.float32), np.zeros(3, np.int64))]   # rank order: A, C (the tie in candidate order), B


def test_yardstick_on_the_hand_made_case():
    """A = (0, 0, 8, 8) score 0.5, B = (2, 0, 10, 8) score 0.25 of the same class (IoU 48 / 80 = 0.6), C = (100, 100, 108, 108) score 0.5, alone; nms 0.45"""
    assert M.iou64(np.array([0, 0, 8, 8.]), np.array([[2, 0, 10, 8.]]))[0] == 0.6
    r, = M.merge_reference(_hand_made(), 0.45, 300)
    assert r["merged"] and r["n"] == 3 and r["kept_before"] == 2 and r["dropped"] == 1
    assert len(r["scores"]) == 1 and r["scores"][0] == 0.5 and r["m"].tolist() == [2]
    np.testing.assert_allclose(r["boxes"][0], [2 / 3, 0, 26 / 3, 8], rtol=0, atol=1e-15)
    r, = M.merge_reference(_hand_made(), 0.45, 300, keep_single=True)
    assert len(r["scores"]) == 2 and r["dropped"] == 0 and r["m"].tolist() == [2, 1]
    np.testing.assert_allclose(r["boxes"][0], [2 / 3, 0, 26 / 3, 8], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(r["boxes"][1], [100, 100, 108, 108])          # C is unchanged
    r, = M.merge_reference(_hand_made(), 0.45, 300, merge=False)
    assert not r["merged"] and len(r["scores"]) == 2
    np.testing.assert_array_equal(r["boxes"], [[0, 0, 8, 8], [100, 100, 108, 108]])
    r, = M.merge_reference(_hand_made(), 0.45, 1)                                # the kept list is cut BEFORE the merge; B still contributes
    assert len(r["scores"]) == 1 and r["m"].tolist() == [2]
    r, = M.merge_reference([tuple(a[:1] for a in _hand_made()[0])], 0.45, 300)   # n = 1: not merged, the single detection stays
    assert not r["merged"] and len(r["scores"]) == 1
    with pytest.raises(AssertionError, match="threshold"):                       # the margin: 0.6 is not exact in fp32
        M.merge_reference(_hand_made(), 0.6, 300)


def _lattice_refs(case, keep_single=False, merge=True, agnostic=None, best=None, classes="case"):
    b0, a0 = M.case_modes(case)
    best, agnostic = b0 if best is None else best, a0 if agnostic is None else agnostic
    classes = case["classes"] if classes == "case" else classes
    return M.merge_reference(M.oracle_candidates(case["pred"], case["thr"], best, classes), case["nms"], case["k"], agnostic, merge, keep_single)


@pytest.mark.parametrize("name", M.LATTICE_CASES)
def test_lattice_cases_are_not_vacuous(name):
    case = M.lattice_case(name)
    ref, single, plain = _lattice_refs(case), _lattice_refs(case, keep_single=True), _lattice_refs(case, merge=False)
    print(name, [(r["n"], r["kept_before"], len(r["scores"]), r["m"].tolist()[:8]) for r in ref])
    M.assert_not_vacuous(ref, name, want_move=name != "zero-weight")
    assert not M.same_detections(ref, plain) and not M.same_detections(ref, single)
    assert all(len(s["scores"]) == p["kept_before"] == len(p["scores"]) for s, p in zip(single, plain))   # KEEP_SINGLE drops nothing
    if name == "contributors":
        assert [int(r["m"][0]) if len(r["m"]) else 1 for r in ref] == list(M.CONTRIBUTORS) and [len(r["scores"]) for r in ref] == [0, 1, 1, 1, 1, 1]
        assert [r["kept_before"] for r in ref] == [2] * 6
    if name == "many-kept":
        assert ref[0]["kept_before"] == 40 > 2 * M.MRG_WAVES and len(ref[0]["scores"]) == 26
    if name == "short-k":
        assert ref[0]["kept_before"] == case["k"] == 4 and len(ref[0]["scores"]) == 3 and len(_lattice_refs(dict(case, k=300), merge=False)[0]["scores"]) == 6
        assert ref[0]["m"].tolist() == [3, 2, 2]
    if name == "shared-box":
        agn = _lattice_refs(case, agnostic=True)
        assert [len(r["scores"]) for r in ref] == [1, 1] and [r["m"].tolist() for r in agn] == [[2, 3], [3]] and not M.same_detections(ref, agn)
        best_agn, best_aware = _lattice_refs(case, agnostic=True, best=True), _lattice_refs(case, best=True)
        assert [r["m"].tolist() for r in best_agn] == [[2], [2]] and [len(r["scores"]) for r in best_aware] == [0, 0]
    if name == "filtered":
        unfiltered = _lattice_refs(case, classes=None)
        assert ref[0]["m"].tolist() == [2] and unfiltered[0]["m"].tolist() == [2, 3]   # the filter removed the only contributor of the first box, and one of the second's
    if name == "zero-area":
        assert ref[0]["dropped"] == 2 and sorted(single[0]["m"].tolist()) == [0, 0, 3]
    if name == "zero-weight":
        assert all(d == 0 for r in single for d in r["den"]) and all((r["moved"] == 0).all() for r in single) and all(r["n"] == 120 for r in ref)
        assert all(0 < len(r["scores"]) < r["kept_before"] for r in ref)
    if name == "global":
        assert case["cap"] // case["n"] < 64 and [r["n"] for r in ref][5] == 0 and max(r["n"] for r in ref) <= 6


def test_bounds_and_truncated_cases_are_what_they_claim():
    case = M.bounds_case()
    cands = M.oracle_candidates(case["pred"], case["thr"])
    assert [len(s) for _, s, _ in cands] == case["counts"] == [0, 1, 2, 2999, 3000]
    ref, plain = M.merge_reference(cands, case["nms"], case["k"]), M.merge_reference(cands, case["nms"], case["k"], merge=False)
    assert [r["merged"] for r in ref] == [False, False, True, True, False]
    assert len(ref[1]["scores"]) == 1                                     # n = 1: the single detection stays
    assert ref[2]["m"].tolist() == [2] and ref[3]["dropped"] > 0 and 0 < len(ref[3]["scores"]) < 300 == ref[3]["kept_before"]
    assert M.same_detections(ref[4:], plain[4:]) and len(ref[4]["scores"]) == 300 and not M.same_detections(ref[3:4], plain[3:4])
    case = M.truncated_case()
    cands = M.oracle_candidates(case["pred"], case["thr"])
    assert [len(s) for _, s, _ in cands] == case["counts"] and case["counts"][0] > 6144   # more than 1.5 * 4096: the score-prefix selection cuts the image


@pytest.mark.parametrize("run", M.GENERAL_RUNS, ids=lambda r: "-".join(map(str, r[:6])))
def test_general_cases_are_not_vacuous(run):
    """on the oracle's own candidates (the kernel tests take the library's decode as operands and tie it to these)"""
    nc, variant, thr, k, best, agnostic, classes = run
    case = M.general_case(run)
    cands = M.oracle_candidates(case["pred"], thr, best, classes)
    ref = M.merge_reference(cands, case["nms"], k, agnostic)
    plain = M.merge_reference(cands, case["nms"], k, agnostic, merge=False)
    print(case["name"], [(r["n"], r["kept_before"], len(r["scores"]), int(r["m"].max()) if len(r["m"]) else 0) for r in ref])
    M.assert_not_vacuous(ref, case["name"])
    assert not M.same_detections(ref, plain)
    assert all(r["n"] < M.MERGE_MAX_N for r in ref)
    if variant == "middle-empty":
        assert ref[1]["n"] == 0 and not ref[1]["merged"]
    if nc > 1 and not best and not classes:
        other = M.merge_reference(cands, case["nms"], k, not agnostic)
        assert not M.same_detections(ref, other), "class-aware and agnostic merge agree"


# ---- the simulator -------------------------------------------------------------------------------------------------------------------------------------------------
def _sim_run(sim, case, flags, nms=None, k=None, rescale=None, slab=False, cap=None):
    """one ymi_postprocess on the simulator: dirty workspace, pre-filled outputs -> outputs (+ slab)"""
    sim.ymi_post_class_mask_offset.argtypes, sim.ymi_post_class_mask_offset.restype = [C.c_int, C.c_int, C.c_int], C.c_int64
    heads, nc, n = case["heads"], case["nc"], case["n"]
    k, cap = k or case["k"], cap or case["cap"]
    logits = _nhwc_logits(heads, nc)
    shapes = [(ho.shape[2], ho.shape[3]) for ho in heads]
    d, out = _post_desc(sim, n, nc, shapes, case["strides"], case["anchors"], case["thr"], case["nms"] if nms is None else nms, k, cap, flags, logits)
    if flags & M.POST_CLASS_FILTER:
        off = int(sim.ymi_post_class_mask_offset(n, sum(3 * h * w for h, w in shapes), cap))
        out["ws"][off: off + 512] = torch.from_numpy(M.K.mask_words(case["classes"]).view(np.uint8).copy())
    if rescale is not None:
        out["rescale"] = torch.tensor(rescale, dtype=torch.float32).reshape(n, 3)
        d.rescale = out["rescale"].data_ptr()
    if slab:
        out["slab"] = torch.full((n, 6 * k + 1), FILL)
        d.out_slab = out["slab"].data_ptr()
    _check(sim, sim.ymi_postprocess(C.byref(d), None))
    return out


def _operands(sim, case, flags, exact):
    """the library's own candidates (nothing suppressed, everything gathered), tied to the oracle's"""
    best, agnostic = bool(flags & M.POST_BEST_CLASS), bool(flags & M.POST_AGNOSTIC)
    oracle = M.oracle_candidates(case["pred"], case["thr"], best, case["classes"] if flags & M.POST_CLASS_FILTER else None)
    out = _sim_run(sim, case, flags & ~(M.POST_MERGE | M.POST_MERGE_KEEP_SINGLE), nms=1.0, k=max(1, max(len(s) for _, s, _ in oracle)))
    assert out["status"][1] == 0
    cands = M.operand_candidates(out)
    M.assert_operands_match_oracle(cands, oracle, exact)
    return cands


def _check_case(sim, case, extra=0, exact=None):
    """merge and merge + KEEP_SINGLE of a case against the yardstick; the unflagged run against the plain top-k; one pass each"""
    exact = case["exact"] if exact is None else exact
    base = case["flags"] | extra
    agnostic = bool(base & M.POST_AGNOSTIC)
    cands = _operands(sim, case, base, exact)
    outs = {}
    for what, f, kw in (("merge", M.POST_MERGE, {}), ("keep-single", M.POST_MERGE | M.POST_MERGE_KEEP_SINGLE, dict(keep_single=True)), ("plain", 0, dict(merge=False))):
        out = _sim_run(sim, case, base | f)
        assert out["status"][1] == 0, out["status"]
        assert int(out["status"][4]) == sum(len(s) for _, s, _ in cands)   # status[4] still counts raw candidates
        M.assert_matches(out, M.merge_reference(cands, case["nms"], case["k"], agnostic, **kw), FILL, exact, f"{case['name']} {what}")
        outs[what] = out
    return outs


@pytest.mark.parametrize("name", M.LATTICE_CASES)
def test_merge_lattice_cases_on_the_simulator(sim, name):
    """shapes 1-3, 5, 7-10: exact operands -> every merged coordinate equals np.float32(num) / np.float32(den) bit for bit"""
    case = M.lattice_case(name)
    lds_before = sim.sim_max_lds()
    outs = _check_case(sim, case)
    assert sim.sim_max_lds() >= 75000 + 16 * min(case["k"], 2999) or lds_before >= 75000   # the merge kernel ran with its dynamic LDS
    if name == "shared-box":   # shapes 5 and 6: agnostic, best-class, both
        for extra in (M.POST_AGNOSTIC, M.POST_BEST_CLASS, M.POST_BEST_CLASS | M.POST_AGNOSTIC):
            _check_case(sim, case, extra)
    if name == "global":
        assert int(outs["merge"]["status"][2]) > 0


def test_merge_eligibility_bounds_on_the_simulator(sim):
    """shape 4: n = 0, 1, 2, 2999, 3000 in one batch; the images outside 1 < n < 3000 are bit-identical to the unflagged run"""
    case = M.bounds_case()
    outs = _check_case(sim, case)
    for key in ("count", "labels", "scores", "boxes"):
        for img in (0, 1, 4):
            assert torch.equal(outs["merge"][key][img], outs["plain"][key][img]) and torch.equal(outs["keep-single"][key][img], outs["plain"][key][img]), (key, img)
    assert outs["merge"]["count"].tolist()[:3] == [0, 1, 1] and outs["merge"]["count"][4] == 300 and outs["merge"]["count"][3] < 300


@pytest.mark.parametrize("run", M.GENERAL_RUNS, ids=lambda r: "-".join(map(str, r[:6])))
def test_merge_general_cases_on_the_simulator(sim, run):
    """boxes and scores through expf: merged coordinates within (2 m + 3) * 2^-24 * max |coordinate| of the float64 mean of the library's own operands"""
    _check_case(sim, M.general_case(run))


def test_merge_rescale_slab_and_stale_rule_on_the_simulator(sim):
    """shape 11: the rescaled output equals fp32 (merged - pad) / gain of the SAME run's unrescaled output bit for bit; the slab equals the four arrays, zero past the
    count; on a capacity overflow every row's count column is YMI_SLAB_STALE"""
    case = M.lattice_case("contributors")
    n, k = case["n"], case["k"]
    rows = [(0.5 + 0.25 * i, 3.0 * i, 7.0 - i) for i in range(n)]
    rows[1] = (0.0, 5.0, 5.0)   # gain 0: no rescale for this image
    for f in (M.POST_MERGE, M.POST_MERGE | M.POST_MERGE_KEEP_SINGLE):
        raw = _sim_run(sim, case, f)
        out = _sim_run(sim, case, f, rescale=rows, slab=True)
        assert torch.equal(raw["count"], out["count"]) and torch.equal(raw["scores"], out["scores"]) and torch.equal(raw["labels"], out["labels"])
        for i, (gain, px, py) in enumerate(rows):
            c = int(out["count"][i])
            b = raw["boxes"][i, :c].numpy()
            want = b if gain == 0 else ((b - np.array([px, py, px, py], np.float32)).astype(np.float32) / np.float32(gain)).astype(np.float32)
            np.testing.assert_array_equal(out["boxes"][i, :c].numpy(), want)
            assert (out["boxes"][i, c:] == FILL).all()
            row = out["slab"][i]
            assert torch.equal(row[: 4 * c], out["boxes"][i, :c].reshape(-1)) and torch.equal(row[4 * k: 4 * k + c], out["scores"][i, :c])
            assert torch.equal(row[5 * k: 5 * k + c], out["labels"][i, :c].float()) and row[6 * k] == c
            assert (row[4 * c: 4 * k] == 0).all() and (row[4 * k + c: 5 * k] == 0).all() and (row[5 * k + c: 6 * k] == 0).all()
        assert any(int(out["count"][i]) > 0 and rows[i][0] != 0 for i in range(n))
    over = _sim_run(sim, case, M.POST_MERGE, slab=True, cap=n * 64)   # 64 records per image: images 4 and 5 (66, 131 candidates) overflow
    assert int(over["status"][1]) & 1 and (over["slab"][:, 6 * k] == -1.0).all()


def test_merge_leaves_a_truncated_image_alone_on_the_simulator(sim):
    """shape 12: the crowded image is cut by the score-prefix selection (4096 <= records < raw count), is never merged (a merged image has fewer than 3000 records, a cut one
    more than 6144) and equals the unflagged run bit for bit, status words included; the small image next to it is merged"""
    case = M.truncated_case()
    plain = _sim_run(sim, case, 0)
    out = _sim_run(sim, case, M.POST_MERGE)
    assert torch.equal(plain["status"], out["status"]), (plain["status"], out["status"])
    st = out["status"].tolist()
    assert st[4] == sum(case["counts"]) and 4096 + 6 <= st[0] < st[4], st        # truncated: fewer records sorted than produced
    for key in ("count", "labels", "scores", "boxes"):
        assert torch.equal(plain[key][0], out[key][0]), key
    assert int(out["count"][0]) == case["k"] and (st[1] & 2) == 0
    cands = M.oracle_candidates(case["pred"], case["thr"])
    ref = M.merge_reference(cands[1:], case["nms"], case["k"])
    M.assert_matches({key: out[key][1:] for key in ("count", "labels", "scores", "boxes")}, ref, FILL, True, "truncated: the small image")
    assert ref[0]["m"].tolist() == [5] and ref[0]["dropped"] == 1 and int(plain["count"][1]) == 2


def test_merge_false_is_identical_to_the_existing_post_cases(sim):
    """without the flag nothing changed: the runs of tests/test_agnostic_nms.py (nc = 2, three images) still equal the oracle, and a run with the flag on images that are all
    outside the merge bound (n = 0 / 1 / 3000 of the bounds case are covered above) is covered by the bitwise checks there"""
    import _head_cases as H
    for variant, thr, k in A.POST_RUNS[:3]:
        heads, strides, anchors, pred = A.post_inputs(2, variant, sim=True)
        case = dict(heads=heads, strides=strides, anchors=anchors, nc=2, n=3, thr=thr, nms=0.45, k=k, cap=3 * 4096, classes=None)
        for flags, agnostic in ((0, False), (M.POST_AGNOSTIC, True)):
            out = _sim_run(sim, case, flags)
            H.assert_equals_oracle(out, A.cut(A.post_full_ref(2, variant, thr, False, agnostic, sim=True), k), FILL)
