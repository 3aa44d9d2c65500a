"""CPU-side checks of the attention op: the C ABI's declarations, the descriptor's layout and the refusals (nothing touches a device), and the constructor contract of
the transformer blocks."""
import ctypes as C
import os
import re
import subprocess

import pytest

import _attn_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from yolort_amd import _build, _lib
    _build.build()
    return _lib.load(require_gpu=False)


def test_header_declares_and_library_exports():
    from yolort_amd import _lib
    src = open(os.path.join(ROOT, "include", "yolort_amd.h")).read()
    assert re.search(r"typedef struct ymi_attn_desc \{.*?\} ymi_attn_desc;", src, re.S)
    for name in ("ymi_attention", "ymi_plan_add_attention"):
        assert re.search(r"\bint %s\(" % name, src) and name in _lib.EXPORTED_SYMBOLS
    assert _lib.ATTN_TILE == tuple(int(re.search(r"#define YMI_ATTN_TILE_%s (\d+)" % a, src).group(1)) for a in "QK")


def test_descriptor_layout_matches_the_c_struct(tmp_path):
    from yolort_amd._lib import AttnDesc
    names = [f for f, _ in AttnDesc._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "yolort_amd.h"\nint main(void) { printf("%zu"' + ', sizeof(ymi_attn_desc)); ' + \
        " ".join('printf(" %%zu", offsetof(ymi_attn_desc, %s));' % f for f in names) + " return 0; }\n"
    (tmp_path / "layout.c").write_text(prog)
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = [int(t) for t in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(AttnDesc)] + [getattr(AttnDesc, f).offset for f in names]


def _desc(**fields):
    """a valid descriptor (2 heads of 32, 4 tokens, fp16) over host memory -- never launched -- with fields overridden"""
    from yolort_amd._lib import AttnDesc
    buf = C.create_string_buffer(4096 + 16)
    base = (C.addressof(buf) + 15) // 16 * 16
    d = AttnDesc(q=base, k=base + 1024, v=base + 2048, o=base + 3072, n=1, S=4, heads=2, d=32, c=64, q_cstride=64, k_cstride=64, v_cstride=64, o_cstride=64, scale=0.5)
    for k, v in fields.items():
        setattr(d, k, v)
    return d, buf


@pytest.mark.parametrize("fields,message", [
    ({"q": None}, b"null"), ({"k": None}, b"null"), ({"v": None}, b"null"), ({"o": None}, b"null"),
    ({"q_cstride": 56}, b">= c"), ({"k_cstride": 0}, b">= c"), ({"v_cstride": 32}, b">= c"), ({"o_cstride": 63}, b">= c"), ({"o_cstride": 68}, b"multiples of 8"),
    ({"c": 96, "q_cstride": 96, "k_cstride": 96, "v_cstride": 96, "o_cstride": 96}, b"heads * d"), ({"heads": 0}, b"heads * d"),
    ({"d": 16, "heads": 4}, b"{32, 64, 128}"), ({"d": 256, "c": 512}, b"{32, 64, 128}"), ({"dtype": 2}, b"F16 or BF16"), ({"S": 0}, b"S >= 1"),
])
def test_refusals_without_a_device(lib, fields, message):
    d, _keep = _desc(**fields)
    good, _keep2 = _desc()
    plan = lib.ymi_plan_create()
    try:
        for rc in (lib.ymi_attention(C.byref(d), None), lib.ymi_plan_add_attention(plan, C.byref(d))):
            assert rc == -1 and message in lib.ymi_last_error() and b"ymi_attention" in lib.ymi_last_error(), lib.ymi_last_error()
        assert lib.ymi_plan_num_ops(plan) == 0
        assert lib.ymi_plan_add_attention(plan, C.byref(good)) == 0 and lib.ymi_plan_num_ops(plan) == 1   # recorded, not launched
    finally:
        lib.ymi_plan_destroy(plan)


def test_constructor_contract():
    """c % heads != 0 and head dimensions outside {32, 64, 128} are refused -- C3TR's four heads therefore need c2 * e in {128, 256, 512}"""
    from yolort_amd.v5 import C3TR, TransformerBlock, TransformerLayer
    assert TransformerBlock(32, 64, 2, 2).out_channels == 64 and TransformerLayer(128, 1).ma.num_heads == 1
    for make in (lambda: TransformerLayer(100, 3), lambda: TransformerLayer(64, 4), lambda: TransformerLayer(512, 2), lambda: TransformerBlock(32, 64, 8, 1), lambda: C3TR(64, 64)):
        with pytest.raises(NotImplementedError):
            make()


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_state_dict_keys_match_the_nn_twin(name):
    m, twin = A.pair(name)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in twin.state_dict().items()]
