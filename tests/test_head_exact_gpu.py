"""The FUSED detection head (yolort_amd/csrc/head_decode.hpp through conv_head_decode_kernel / conv_head_decode_group_kernel: the 1x1 head convolution with sigmoid,
anchor decode, multi-label threshold and candidate compaction in its epilogue) against the oracle on CHOSEN inputs whose logits are exact (tests/_head_cases.py): the
expected detections are O.postprocess(O.decode(logits)) computed from those logits alone, with no convolution error to budget.

Reached on purpose, and asserted from the oracle's decode before anything runs: the worklist spill and the record-buffer flush (more than HdCfg::BUF records in one wave,
at the start of a level, across an image boundary and ending at pixel M - 1), the image change inside an append, the pre-filter at exact score ties, at an objectness one
ulp above the threshold, at saturated class logits and at thresholds <= 0, the padding channels at every anchor padding, the group launch over 1 ... 4 levels, the
per-level launch, the global candidate sink, the overflow report -- and, in a fresh child process with YOLORT_AMD_HEAD_SPLIT=0, the NA = 3 instantiations."""
import base64
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _head_cases as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -3.0
KEYS = ("count", "labels", "scores", "boxes")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test run on a host without a GPU")
    return torch.device("cuda:0")


_RESULTS = {}


def _forms(dev, name):
    """the three forms of a case (shared by the tests that need them, left unchanged)"""
    if name not in _RESULTS:
        case = H.head_case(name)
        _RESULTS[name] = {mode: H.gpu_head(dev, case, mode, FILL) for mode in H.HEAD_MODES}
    return _RESULTS[name]


@pytest.mark.parametrize("name", H.GPU_CASES)
def test_fused_head_equals_the_oracle_on_exact_logits(dev, name):
    """group launch, per-level launches and the stored-logits post-process of one case: the fused result equals the oracle (counts, labels, order exact; scores rtol 2e-6 /
    atol 1e-7, boxes rtol 1e-5 / atol 1e-4; slots past the count keep their fill), the three forms agree bit for bit (the header of head_decode.hpp claims exactly this),
    status word 0 included.  With nms_thresh = 1.0 and k above the candidate count (all cases but `nms`) nothing is suppressed or cut: the box of EVERY candidate anchor is
    compared.  Palette cases: the scores are bit-equal to 0.25, 0.5 or 1.0."""
    case, ref = H.head_case(name), H.head_reference(name)
    print(H.assert_head_case_is_not_vacuous(case, ref))
    got = _forms(dev, name)
    for mode in H.HEAD_MODES:
        print(mode, "passes", got[mode]["passes"], "cap", got[mode]["cap"])
    H.assert_equals_oracle(got["group"], ref, FILL)
    for mode in ("single", "unfused"):
        for key in KEYS:
            assert torch.equal(got[mode][key], got["group"][key]), f"{mode} differs from the group launch in {key}"
        assert got[mode]["passes"][-1][0] == got["group"]["passes"][-1][0], (mode, got[mode]["passes"], got["group"]["passes"])
        assert got[mode]["cap"] == got["group"]["cap"]
    if case["design"].startswith("palette"):
        for i in range(case["n"]):
            s = got["group"]["scores"][i, : int(got["group"]["count"][i])]
            assert torch.isin(s, torch.tensor([0.25, 0.5, 1.0])).all(), s
            assert bool((s > case["thr"]).all())
    if case["expect_candidates"] is not None:
        assert int(got["group"]["count"].sum()) == case["expect_candidates"]
    if "overflow" in case["guards"]:   # the first pass reports the overflow (YMI_STATUS bit 0), the protocol grows the capacity and redoes the batch
        for mode in H.HEAD_MODES:
            assert got[mode]["passes"][0][1] & 1 and len(got[mode]["passes"]) > 1 and got[mode]["cap"] > case["cand_cap"], (mode, got[mode]["passes"])
    if "global-sink" in case["guards"]:   # the global list held everything: one pass at the initial capacity
        for mode in H.HEAD_MODES:
            assert len(got[mode]["passes"]) == 1 and got[mode]["cap"] == case["cand_cap"], (mode, got[mode]["passes"])
            assert got[mode]["passes"][0][0] == int(case["cand"].sum())


_CHILD = r"""
import base64, io, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import _head_cases as H
dev = torch.device("cuda:0")
for name in sys.argv[1:]:
    case = H.head_case(name)
    for mode in ("group", "single"):
        got = H.gpu_head(dev, case, mode, %r)
        buf = io.BytesIO()
        np.savez_compressed(buf, **{k: got[k].numpy() for k in ("count", "labels", "scores", "boxes")})
        print("DET", name, mode, base64.b64encode(buf.getvalue()).decode(), flush=True)
print("DONE")
"""


def test_three_anchors_per_wave_equal_the_oracle_and_the_anchor_split_form(dev):
    """YOLORT_AMD_HEAD_SPLIT=0 (read once per process: a fresh child) selects the NA = 3 instantiations -- a wave holds all three anchors, HdCfg<3>: BUF = 1024, WL = 512,
    ring depth 3 -- which no other test runs: the dense case, one tie case and one class count per TNA through both launches.  The child prints its detections; they equal
    the oracle and this process's NA = 1 results bit for bit."""
    for name in H.NA3_CASES:
        case = H.head_case(name)
        H.assert_head_case_is_not_vacuous(case, H.head_reference(name))
    assert "buf-na3" in H.head_case("dense")["guards"] and {(H.head_case(nm)["nc"] + 36) // 32 for nm in H.NA3_CASES} >= {1, 2, 3, 4}
    env = dict(os.environ, YOLORT_AMD_HEAD_SPLIT="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), FILL), *H.NA3_CASES], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("DONE"), (r.returncode, r.stderr[-3000:])
    seen = set()
    for line in r.stdout.splitlines():
        if not line.startswith("DET "):
            continue
        _, name, mode, blob = line.split(" ", 3)
        z = np.load(io.BytesIO(base64.b64decode(blob)))
        got = {k: torch.from_numpy(z[k]) for k in KEYS}
        H.assert_equals_oracle(got, H.head_reference(name), FILL)
        mine = _forms(dev, name)["group"]
        for key in KEYS:
            assert torch.equal(got[key], mine[key]), f"{name} / {mode}: NA = 3 differs from NA = 1 in {key}"
        seen.add((name, mode))
    assert seen == {(name, mode) for name in H.NA3_CASES for mode in ("group", "single")}, seen
