"""Cases and the float64 yardstick of the int8 convolution tests (test_conv_i8.py, test_conv_i8_gpu.py).

Which case reaches which code path of csrc/conv_i8.hip (k = 1: tiles of 128 raster pixels, chunks of four k32 steps = 128 channels; k = 3: tiles of 8 x 16 outputs of
one image, chunks of 32 channels; both: slabs of 64 output channels as two 32-wide accumulator tiles):
  k1_tiny_distinct            less than one tile both ways, one k32 step whose second half is padding; distinct weight per (co, ci): the K order inside a lane's 16 bytes
                              and the transposed accumulator layout
  k1_odd_packets_cout_tail    3 packets (odd), 260 pixels = two tiles + 4, cout 72 = one slab + a slab of one partly filled accumulator tile
  k1_s2_three_chunks          17 packets = 9 steps = two chunks + one step, stride 2 (the pixel decode), a pixel tile that spans both images, cout 40 = 32 + 8
  k3_s1_borders_two_images    four borders and corners, 2 x 2 spatial tiles per image (9 x 19), two channel chunks the second half padding, distinct weights per tap
  k3_s2_odd / k3_s2_even      9 x 11 -> 5 x 6 and 8 x 8 -> 4 x 4: odd and even extents, the last window half outside
  k3_s2_four_tiles            19 x 35 -> 10 x 18: 2 x 2 tiles at stride 2, two slabs
  k3_extremes                 cin 512 (16 chunks), |x| = |w| = 127 in sign patterns: acc = +-7.4e7 > 2^24 and odd, so the conversion rounds; with out_scale 0.25 half of the
                              outputs clamp, at both ends
With spatial tiles per image no k = 3 tile holds an image change; k1_s2_three_chunks has one inside a k = 1 tile.
"""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_SILU, ACT_HARDSWISH, ACT_LEAKY = 0, 1, 2, 3
U = 2.0 ** -24   # unit roundoff of fp32

# name: (n, h, w, cin, cout, k, s, fill)
CONV_CASES = {
    "k1_tiny_distinct": (1, 5, 7, 16, 8, 1, 1, "distinct"),
    "k1_odd_packets_cout_tail": (1, 13, 20, 48, 72, 1, 1, "random"),
    "k1_s2_three_chunks": (2, 9, 11, 272, 40, 1, 2, "random"),
    "k3_s1_borders_two_images": (2, 9, 19, 48, 40, 3, 1, "distinct"),
    "k3_s2_odd": (1, 9, 11, 32, 16, 3, 2, "random"),
    "k3_s2_even": (1, 8, 8, 32, 16, 3, 2, "distinct"),
    "k3_s2_four_tiles": (1, 19, 35, 32, 72, 3, 2, "random"),
    "k3_extremes": (1, 4, 5, 512, 8, 3, 1, "extreme"),
}
EPILOGUE_SHAPE = (1, 6, 7, 32, 24, 3, 1, "random")   # act x output type x shortcut run on this one


def operands(case, seed=0):
    """(xq int8 NCHW, wq int8 OIHW, scale fp32 [cout], bias fp32 [cout]) of a case, on the CPU.  "distinct": weights that differ per (co, ci, tap), power-of-two scale and
    bias so that an identity epilogue is exact; "extreme": see the module docstring; "random": full-range codes, scales that put the pre-activations at a few units."""
    n, h, w, cin, cout, k, s, fill = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-127, 128, (n, cin, h, w), generator=g)
    co, ci, tap = torch.arange(cout).view(-1, 1, 1), torch.arange(cin).view(1, -1, 1), torch.arange(k * k).view(1, 1, -1)
    if fill == "distinct":
        wt = (31 * ci + 7 * tap + 13 * co) % 255 - 127
        scale, bias = torch.full((cout,), 2.0 ** -10), torch.arange(cout).float() - cout // 2
    elif fill == "extreme":
        sign = 1 - 2 * (ci % 2)
        x = (127 * sign.view(1, -1, 1, 1)).expand(n, cin, h, w).clone()
        x[:, 0] = 126   # makes the sums odd: above 2^24 the conversion to fp32 has to round
        wt = 127 * sign * (1 - 2 * (co % 2)) * torch.ones_like(tap)
        wt = torch.where(co >= 4, torch.randint(0, 2, (cout, cin, k * k), generator=g) * 254 - 127, wt)
        scale, bias = torch.full((cout,), 1e-6), torch.zeros(cout)
    else:
        wt = torch.randint(-127, 128, (cout, cin, k * k), generator=g)
        scale = 3.0 / (73.0 * 73.0 * (cin * k * k) ** 0.5) * (1 + torch.arange(cout) / cout)
        bias = torch.randn(cout, generator=g)
    return x.to(torch.int8), wt.reshape(cout, cin, k, k).to(torch.int8), scale.float(), bias.float()


def reference(xq, wq, scale, bias, k, s, act, res=None, res_scale=1.0):
    """(the float64 value before the final rounding, the bound on the fp32 epilogue's error against it), NCHW.  The integer convolution is F.conv2d in float64: every
    partial sum is an integer below 2^53, so it is exact in any order.  The bound is the one derived in test_conv_i8_gpu.py's docstring."""
    acc = F.conv2d(xq.double(), wq.double(), None, s, k // 2)
    sc, bi = scale.double().view(1, -1, 1, 1), bias.double().view(1, -1, 1, 1)
    pre = acc * sc + bi
    err = U * ((acc * sc).abs() + pre.abs())
    if act == ACT_SILU:
        a = pre * torch.sigmoid(pre)
        err = 1.1 * err + (6 + pre.abs()) * U * a.abs()
    elif act == ACT_HARDSWISH:
        a = pre * torch.clamp(pre + 3, 0, 6) / 6
        err = 1.5 * err + 4 * U * a.abs()
    elif act == ACT_LEAKY:
        a = torch.where(pre > 0, pre, pre * 0.1)
        err = err + 2 * U * a.abs()
    else:
        a = pre
    post = a if res is None else a + float(torch.tensor(res_scale, dtype=torch.float32)) * res.double()
    return post, err + U * post.abs()


def check_int8(got, post, err, out_scale):
    """exact codes, except one code of slack where the float64 code lies within the derived bound of a half-integer; at most 1 % of the elements may be such"""
    code = post / out_scale
    delta = err / out_scale + 2 * U * code.abs()
    want = torch.clamp(torch.round(code), -127, 127)
    excused = ((code - torch.floor(code) - 0.5).abs() <= delta) & (code.abs() < 128)
    diff = (got.double().cpu() - want).abs()
    bad = (diff > 0) & ~(excused & (diff <= 1))
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} codes differ; first at {bad.nonzero()[0].tolist()}: got {got.cpu()[bad][0]}, float64 code {code[bad][0]}"
    assert float(excused.double().mean()) <= 0.01, f"{float(excused.double().mean()):.4f} of the elements sit on a rounding boundary"


def check_16(got, post, err, dtype):
    """one rounding of the 16-bit type (half a spacing at the reference) plus the derived fp32 bound"""
    from _exact import spacing
    tol = 0.5 * spacing(post, dtype) + err
    over = (got.double().cpu() - post).abs() > tol * (1 + 1e-12)
    assert not bool(over.any()), f"{int(over.sum())} of {over.numel()} elements off by more than one rounding; first at {over.nonzero()[0].tolist()}: got {got.cpu()[over][0]}, want {post[over][0]}"


def quantize_reference(x, scale):
    """float64 rint + clip of x / scale (NaN -> 0): bit for bit when the scale is a power of two"""
    q = torch.clamp(torch.round(x.double() / scale), -127, 127)
    return torch.where(torch.isnan(q), torch.zeros_like(q), q).to(torch.int8)
