"""The NV12 letterbox kernels of csrc/preproc_nv12.hip on the CPU simulator (tests/hipsim): a lean twin of tests/test_nv12_gpu.py -- every case of tests/_nv12_cases.py
under the default dispatch (the per-pixel kernel) and two forced tile shapes, and the refusals (host code)."""
import ctypes as C
import os
import subprocess

import pytest

import _nv12_cases as N
from test_hipsim_kernels import SIM_DIR, _clangxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_VARIANTS = (("default", None, None), ("4-cg1", "4", "1"), ("2-cg2", "2", "2"))


@pytest.fixture(scope="module")
def sim():
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no host clang++ (ext_vector_type / _Float16 / __bf16 sources need clang)")
    out_dir = os.path.join(SIM_DIR, "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libhipsim_nv12.so")
    srcs = [os.path.join(SIM_DIR, f) for f in ("hipsim.h", "hipsim.cpp", "sim_kernels_nv12.cpp")] + [os.path.join(ROOT, "yolort_amd", "csrc", f) for f in ("preproc_nv12.hip", "common.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs + [os.path.join(ROOT, "include", "yolort_amd.h")]):
        subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-I", SIM_DIR, "-I", os.path.join(ROOT, "include"), "-Wno-unused-function", "-Wno-psabi",
                        srcs[2], "-o", so], check=True)
    lib = C.CDLL(so)
    lib.sim_last_error.restype = C.c_char_p
    lib.ymi_letterbox_nv12.restype, lib.ymi_letterbox_nv12.argtypes = N._lib._SIGS["ymi_letterbox_nv12"]
    lib.ymi_nv12_to_rgb.restype, lib.ymi_nv12_to_rgb.argtypes = N._lib._SIGS["ymi_nv12_to_rgb"]
    return lib


@pytest.mark.parametrize("name", [c.name for c in N.CASES])
def test_letterbox_nv12_equals_the_model_bit_for_bit(sim, name):
    N.check(sim, N.BY_NAME[name], variants=SIM_VARIANTS)


def test_refusals(sim):
    N.check_refusals(sim, "cpu")
