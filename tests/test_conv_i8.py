"""CPU-side checks of the int8 convolution: the C ABI's declarations, layouts and refusals (nothing touches a device), the weight blob against its stated layout,
the quantisation of PackedConvI8 and the constructor contract of QConv."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("ymi_conv2d_i8", "ymi_plan_add_conv_i8", "ymi_quantize_i8", "ymi_plan_add_quantize_i8", "ymi_conv_i8_pack_bytes", "ymi_conv_i8_pack")


@pytest.fixture(scope="module")
def lib():
    from yolort_amd import _build, _lib
    _build.build()
    return _lib.load(require_gpu=False)


def test_header_declares_and_library_exports(lib):
    from yolort_amd import _lib
    src = open(os.path.join(ROOT, "include", "yolort_amd.h")).read()
    for struct in ("ymi_conv_i8_desc", "ymi_quant_i8_desc"):
        assert re.search(r"typedef struct %s \{.*?\} %s;" % (struct, struct), src, re.S)
    for name in FUNCS:
        assert re.search(r"\bint(64_t)? %s\(" % name, src) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.ymi_abi_version() == 6


def test_descriptor_sizes_match_the_header(tmp_path):
    from yolort_amd import _lib
    (tmp_path / "s.c").write_text('#include <stdio.h>\n#include "yolort_amd.h"\nint main(){printf("%zu %zu\\n", sizeof(ymi_conv_i8_desc), sizeof(ymi_quant_i8_desc));return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(_lib.ConvI8Desc), C.sizeof(_lib.QuantI8Desc)]


def _descs(conv=None, quant=None):
    """valid descriptors (16 -> 8 channels, 4 x 4, k3 s1, int8 out; 64 x 16 fp16 values) over host memory -- never launched -- with fields overridden"""
    from yolort_amd._lib import ConvI8Desc, QuantI8Desc
    buf = C.create_string_buffer(8192 + 16)
    base = (C.addressof(buf) + 15) // 16 * 16
    d = ConvI8Desc(x=base, w=base + 1024, scale=base + 4096, bias=base + 5120, y=base + 6144, n=1, h=4, w_in=4, cin=16, x_cstride=16, ho=4, wo=4, cout=8, y_cstride=8,
                   k=3, s=1, p=1, out_dtype=5, out_scale=0.5, res_scale=1.0)
    q = QuantI8Desc(x=base, y=base + 4096, npix=64, c=16, x_cstride=16, y_cstride=16, dtype=0, scale=0.5)
    for k, v in (conv or {}).items():
        setattr(d, k, v)
    for k, v in (quant or {}).items():
        setattr(q, k, v)
    return d, q, buf


@pytest.mark.parametrize("op,fields,message", [
    ("conv", {"x": None}, b"null"), ("conv", {"w": None}, b"null"), ("conv", {"scale": None}, b"null"), ("conv", {"bias": None}, b"null"), ("conv", {"y": None}, b"null"),
    ("conv", {"cin": 24, "x_cstride": 32}, b"multiple of 16"), ("conv", {"cout": 12, "y_cstride": 16}, b"multiple of 8"), ("conv", {"k": 5, "p": 2}, b"k in {1, 3}"),
    ("conv", {"s": 3, "ho": 2, "wo": 2}, b"s in {1, 2}"), ("conv", {"x_cstride": 0}, b">= c"), ("conv", {"y_cstride": 4}, b">= c"), ("conv", {"res": 1 << 20, "res_cstride": 0}, b">= c"),
    ("conv", {"out_dtype": 2}, b"I8, F16 or BF16"), ("conv", {"out_scale": 0.0}, b"out_scale > 0"), ("conv", {"out_scale": -1.0}, b"out_scale > 0"), ("conv", {"act": 4}, b"unknown activation"),
    ("conv", {"ho": 5}, b"does not follow"),
    ("quant", {"x": None}, b"null"), ("quant", {"y": None}, b"null"), ("quant", {"dtype": 3}, b"F16, BF16 or F32"), ("quant", {"c": 0}, b"bad extent"), ("quant", {"x_cstride": 8}, b">= c"),
    ("quant", {"y_cstride": 8}, b">= c"), ("quant", {"scale": 0.0}, b"scale must be"), ("quant", {"scale": float("nan")}, b"scale must be"),
])
def test_refusals_without_a_device(lib, op, fields, message):
    pick = (lambda t: t[0]) if op == "conv" else (lambda t: t[1])
    direct, add, name = (lib.ymi_conv2d_i8, lib.ymi_plan_add_conv_i8, b"ymi_conv2d_i8") if op == "conv" else (lib.ymi_quantize_i8, lib.ymi_plan_add_quantize_i8, b"ymi_quantize_i8")
    bad_all, good_all = _descs(**{op: fields}), _descs()
    plan = lib.ymi_plan_create()
    try:
        for rc in (direct(C.byref(pick(bad_all)), None), add(plan, C.byref(pick(bad_all)))):
            assert rc == -1 and message in lib.ymi_last_error() and name in lib.ymi_last_error(), lib.ymi_last_error()
        assert lib.ymi_plan_num_ops(plan) == 0
        assert add(plan, C.byref(pick(good_all))) == 0 and lib.ymi_plan_num_ops(plan) == 1   # recorded, not launched
    finally:
        lib.ymi_plan_destroy(plan)


@pytest.mark.parametrize("cout,cin,k", [(8, 16, 1), (72, 48, 1), (40, 48, 3)])
def test_pack_matches_the_stated_layout(lib, cout, cin, k):
    """blob[tap][p][co][j] = w[co][16 p + j][ky][kx], zero where p >= cin / 16 or co >= cout (include/yolort_amd.h), on weights distinct per (co, ci, tap)"""
    w = ((np.arange(cout * cin * k * k, dtype=np.int64) * 37) % 255 - 127).astype(np.int8).reshape(cout, cin, k, k)
    P, P2, CP = cin // 16, (cin // 16 + 1) // 2 * 2, (cout + 31) // 32 * 32
    want = np.zeros((k * k, P2, CP, 16), dtype=np.int8)
    want[:, :P, :cout] = w.reshape(cout, P, 16, k * k).transpose(3, 1, 0, 2)
    assert lib.ymi_conv_i8_pack_bytes(cout, cin, k) == want.size and lib.ymi_conv_i8_pack_bytes(cout, cin + 8, k) == -1 and lib.ymi_conv_i8_pack_bytes(cout, cin, 5) == -1
    blob = np.full(want.size, 99, dtype=np.int8)
    assert lib.ymi_conv_i8_pack(w.ctypes.data, cout, cin, k, blob.ctypes.data, blob.size) == 0
    assert np.array_equal(blob.reshape(want.shape), want)
    assert lib.ymi_conv_i8_pack(w.ctypes.data, cout, cin, k, blob.ctypes.data, blob.size - 1) == -1 and b"ymi_conv_i8_pack" in lib.ymi_last_error()


def test_packed_conv_i8_quantises_within_half_a_step(lib):
    from yolort_amd.engine import PackedConvI8
    g = torch.Generator().manual_seed(3)
    w = torch.randn(24, 32, 3, 3, generator=g)
    w[5] = 0.0   # an all-zero row: its scale is 1, not 0 / 0
    bn = (torch.rand(24, generator=g) + 0.5, torch.randn(24, generator=g), torch.randn(24, generator=g), torch.rand(24, generator=g) + 0.1, 1e-3)
    pc = PackedConvI8(w, None, bn, 0.02, torch.device("cpu"))
    fold = bn[0].double() / torch.sqrt(bn[3].double() + 1e-3)
    w64 = w.double() * fold.view(-1, 1, 1, 1)
    assert pc.wq.dtype == torch.int8 and int(pc.wq.abs().max()) == 127 and float(pc.w_scale[5]) == 1.0 and not bool(pc.wq[5].any())
    assert bool(((pc.wq.double() * pc.w_scale.view(-1, 1, 1, 1) - w64).abs() <= 0.5 * pc.w_scale.view(-1, 1, 1, 1) * (1 + 1e-12)).all())
    assert torch.equal(pc.scale, (0.02 * pc.w_scale).float()) and torch.equal(pc.bias, (bn[1].double() - bn[2].double() * fold).float())
    assert pc.w.numel() == lib.ymi_conv_i8_pack_bytes(24, 32, 3)


def test_qconv_constructor_contract(lib):
    from yolort_amd.v5 import Conv, QConv
    q = QConv.from_float(Conv(16, 8, 3, 2).eval(), 0.05, 0.1)
    assert sorted(q.state_dict()) == ["bias", "in_scale", "out_scale", "w_scale", "wq"] and q.wq.dtype == torch.int8 and float(q.out_scale) == 0.1
    assert float(QConv.from_float(Conv(16, 8, 1).eval(), 0.05).out_scale) == 0.0
    for conv in (Conv(16, 16, 3, g=16).eval(), Conv(16, 8, 5).eval(), Conv(16, 8, 3)):   # depthwise, k = 5, training mode
        with pytest.raises(NotImplementedError):
            QConv.from_float(conv, 0.05)
