"""CPU-side checks of the depthwise convolution: the C ABI's declarations and refusals (nothing touches a device) and the constructor contract of the blocks."""
import ctypes as C
import os
import re

import pytest

import _ghost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from yolort_amd import _build, _lib
    _build.build()
    return _lib.load(require_gpu=False)


def test_header_declares_and_library_exports():
    from yolort_amd import _lib
    src = open(os.path.join(ROOT, "include", "yolort_amd.h")).read()
    assert re.search(r"typedef struct ymi_dwconv_desc \{.*?\} ymi_dwconv_desc;", src, re.S)
    for name in ("ymi_dwconv2d", "ymi_plan_add_dwconv"):
        assert re.search(r"\bint %s\(" % name, src) and name in _lib.EXPORTED_SYMBOLS


def _desc(**fields):
    """a valid descriptor (8 channels, 4 x 4, k3 s1, fp16) over host memory -- never launched -- with fields overridden"""
    from yolort_amd._lib import DwConvDesc
    buf = C.create_string_buffer(4096 + 16)
    base = (C.addressof(buf) + 15) // 16 * 16
    d = DwConvDesc(x=base, w=base + 1024, bias=base + 2048, y=base + 3072, n=1, h=4, w_in=4, c=8, x_cstride=8, y_cstride=8, ho=4, wo=4, k=3, s=1, p=1)
    for k, v in fields.items():
        setattr(d, k, v)
    return d, buf


@pytest.mark.parametrize("fields,message", [
    ({"c": 12, "x_cstride": 16, "y_cstride": 16}, b"multiple of 8"), ({"k": 7, "p": 3}, b"k in {3, 5}"), ({"k": 1, "p": 0}, b"k in {3, 5}"), ({"s": 3, "ho": 2, "wo": 2}, b"s in {1, 2}"),
    ({"dtype": 2}, b"F16 or BF16"), ({"x_cstride": 0}, b">= c"), ({"y_cstride": 4}, b">= c"), ({"res": 1 << 20, "res_cstride": 0}, b">= c"),
    ({"x": None}, b"null"), ({"w": None}, b"null"), ({"bias": None}, b"null"), ({"y": None}, b"null"),
])
def test_refusals_without_a_device(lib, fields, message):
    d, _keep = _desc(**fields)
    good, _keep2 = _desc()
    plan = lib.ymi_plan_create()
    try:
        for rc in (lib.ymi_dwconv2d(C.byref(d), None), lib.ymi_plan_add_dwconv(plan, C.byref(d))):
            assert rc == -1 and message in lib.ymi_last_error() and b"ymi_dwconv2d" in lib.ymi_last_error(), lib.ymi_last_error()
        assert lib.ymi_plan_num_ops(plan) == 0
        assert lib.ymi_plan_add_dwconv(plan, C.byref(good)) == 0 and lib.ymi_plan_num_ops(plan) == 1   # recorded, not launched
    finally:
        lib.ymi_plan_destroy(plan)


def test_constructor_contract():
    from yolort_amd.v5 import Conv, DWConv
    assert Conv(16, 16, 3, g=16).conv.groups == 16
    for make in (lambda: Conv(16, 32, 3, g=2), lambda: DWConv(16, 32, 3), lambda: DWConv(16, 16, 1)):
        with pytest.raises(NotImplementedError):
            make()


@pytest.mark.parametrize("name", sorted(_ghost.CASES))
def test_state_dict_keys_match_the_nn_twin(name):
    m, twin = _ghost.pair(name)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in twin.state_dict().items()]
