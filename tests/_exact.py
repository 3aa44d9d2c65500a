"""Per-element checks of the convolution kernels on EXACTLY REPRESENTABLE operands (helpers, no fixtures; used by
tests/test_conv_exact_gpu.py on the GPU and by tests/test_hipsim_kernels.py on the CPU lane simulator).

The max-norm bound of the parity tests (2e-3 / 1.6e-2 of the largest output) leaves room for a truncating pack, a double
rounding, a 16-bit bias or a wrong tap at a border pixel.  Here the operands are chosen so that the fp32 accumulation is EXACT in
any order (see `exact_operands`), which makes the float64 reference, rounded once to the storage type, the one right answer:
  * act = none   the output must be bit-identical to it (accumulate, bias in fp32, shortcut added in fp32 before the ONE rounding,
                 round-to-nearest-even);
  * SiLU         every element within `max_ulp` units of the storage type's spacing, and the mean SIGNED error (towards / away
                 from zero) within 0.1 ulp -- a truncating pack shows as about -0.5.
"""
import functools

import torch
import torch.nn.functional as F

MANT_BITS = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}    # stored fraction bits
MIN_EXP = {torch.float16: -14, torch.bfloat16: -126, torch.float32: -126}   # exponent of the smallest normal number

A_MAX, W_MAX, W_DEN = 3, 2, 8          # activations: integers in [-3, 3]; weights: integers in [-2, 2] / 8
K_MAX = 9 * 128                        # the longest reduction any case here runs (3x3 over 128 channels)
BIAS_MAX, RES_MAX = 4096.0, 8.0        # |bias| (a multiple of 1/8), |shortcut| (a multiple of 1/4, representable in bf16)

# (n, h, w): all taps but the centre are padding / one-row and one-column maps / smaller than the 3x3 window's span / ragged / several partial tiles
SHAPES = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 3, 3), (3, 5, 4), (1, 17, 33)]
WIDTHS = [(32, 32), (64, 128), (64, 40), (128, 64), (48, 96)]   # (cin, cout); 48 -> 96: the im2col-table form (cin % 32 != 0)
KINDS = [(1, 1), (3, 1), (3, 2)]                                # (kernel, stride), pad = kernel // 2

# kernel families by the tile ids of the existing parametrisations: name -> (tile ids, (kernel, stride) kinds, extra widths)
FAMILIES = {
    "v2": ([12, 21, 24, 27, 61, 64, 66], KINDS, []),                      # 4-wave LDS-DMA implicit GEMM (conv_igemm_impl.hpp)
    "v1": ([-1, -2, -3, -4, -5], KINDS, []),                              # register-staged kernel (negative ids)
    "igemm8": ([111, 112, 113, 114, 115, 116], KINDS, []),                # 8-wave implicit GEMM (conv_igemm8.hip)
    "halo": ([31, 32, 33, 34, 35, 36, 37], [(3, 1)], []),                 # LDS-halo 3x3 (conv3x3_halo.hip)
    "halo8": ([91, 92, 93, 94, 95], [(3, 1)], []),                        # 8-wave LDS-halo 3x3 (conv_halo8.hip)
    "stream": ([121, 122, 123, 124], [(1, 1)], []),                       # streaming 1x1 (conv1x1_stream.hip)
    "tp": ([141, 142, 143, 144, 145, 151, 152, 155], KINDS, []),   # row-transposed stores (the 15x range has no variants 13 / 14: refused)
    "c32": ([131], [(3, 1), (3, 2)], []),                                 # conv3x3_c32.hip
    "res": ([132, 133], [(3, 1)], [(64, 64)]),                            # conv3x3_res.hip / conv3x3_rw.hip
    "rw2": ([134], [(3, 2)], []),                                         # conv3x3_rw2.hip, 64 -> 128
    "rw3": ([135], [(3, 2)], [(128, 128)]),                               # ... its K-split form, cin = 128
    "rs": ([137, 138], [(3, 1), (3, 2)], [(64, 64)]),                     # conv3x3_rs.hip
    "rule": ([0], KINDS, []),                                             # the library's own choice
}
F32_TILES = [201, 202, 203, 204, 205, 206]
NO_SHORTCUT = (134, 135, 137, 138)      # tiles without a shortcut input (their launches are given none)
SILU_ONLY = (133, 134, 135, 137, 138)   # tiles whose launchers take SiLU only: an identity-activation launch is refused (the plan's rules then pick another tile)


def family_of(tile):
    for name, (tiles, _, _) in FAMILIES.items():
        if tile in tiles:
            return name
    raise KeyError(tile)


def cases(tile, shapes=SHAPES, widths=None):
    """(n, h, w, cin, cout, k, s) of every case a tile is given: its family's kinds x shapes x widths"""
    _, kinds, extra = FAMILIES[family_of(tile)] if tile not in F32_TILES else (None, KINDS, [])
    out = []
    for (k, s) in kinds:
        for (n, h, w) in shapes:
            for (cin, cout) in (WIDTHS + extra if widths is None else widths):
                out.append((n, h, w, cin, cout, k, s))
    return out


def group_of(case):
    """the group of a case's launches for the mean signed error: the small maps, or the one large map"""
    return "large map" if tuple(case[:3]) == SHAPES[-1] else "small maps"


def out_hw(h, w, k, s):
    p = k // 2
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


@functools.lru_cache(maxsize=None)
def exact_operands(n, h, w, cin, cout, k, s, seed=0):
    """x (n, cin, h, w), weight (cout, cin, k, k), bias (cout), shortcut (n, cout, ho, wo): float64 tensors (shared between the
    tests: do not modify) whose values every storage type holds exactly, such that the kernels' fp32 arithmetic is exact too.

    Bound: activations are integers a with |a| <= 3, weights are q / 8 with integer |q| <= 2, so every product is an integer
    multiple of 1/8 of magnitude <= 3 * 2 / 8 = 3/4, and a sum of any subset of the K <= 9 * 128 = 1152 products of one output is a
    multiple of 1/8 of magnitude <= 864.  The bias (a multiple of 1/8, |b| <= 4096; held in fp32 by the library) and the shortcut
    (a multiple of 1/4, |r| <= 8) keep every partial sum a multiple of 1/8 below 864 + 4096 + 8 < 2^13, i.e. an integer below
    2^16 in units of 1/8 -- far inside the 2^24 consecutive integers fp32 holds.  Every partial sum is therefore exact whatever the
    order of the additions: the MFMA adder tree, a K split over waves and the simulator's fixed order all give the same number.

    Weight pattern: output channel o < k * k * 3 carries ONE non-zero weight -- tap (o // 3) of input channel {0, cin // 2, cin - 1}
    [o % 3] -- so a dropped, duplicated or shifted tap changes an exactly known integer multiple of 1/8 at every pixel, border
    pixels included; the next channels are sparse (pre-activations of a few units: the curved part of SiLU), the last two dense
    (the full-length accumulation, |v| up to a few dozen).  Every fourth bias is large: those outputs need the rounding in 16 bits."""
    assert cin * k * k <= K_MAX, "the exactness bound is derived for K <= 9 * 128"
    g = torch.Generator().manual_seed(1000 * seed + 97 * cin + 13 * cout + 7 * h + 3 * w + k + s)
    ho, wo = out_hw(h, w, k, s)
    x = torch.randint(-A_MAX, A_MAX + 1, (n, cin, h, w), generator=g).double()
    q = torch.randint(-W_MAX, W_MAX + 1, (cout, cin, k, k), generator=g)
    ntap = min(k * k * 3, cout - 2)
    keep = torch.rand(cout, cin, k, k, generator=g) < min(1.0, 24.0 / (cin * k * k))
    keep[-2:] = True
    q = q * keep
    q[:ntap] = 0
    for o in range(ntap):
        tap, ci = o // 3, (0, cin // 2, cin - 1)[o % 3]
        q[o, ci, tap // k, tap % k] = (1, -2, 2)[o % 3] * (1 if (o // 3) % 2 == 0 else -1)
    wt = q.double() / W_DEN
    bias = torch.randint(-16, 17, (cout,), generator=g).double() / 8
    big = torch.tensor([1000.125, -2049.625, 33.125, -515.625, 4095.875, -1027.375], dtype=torch.float64)   # (negative ones far below -88.7: see reference64)
    bias[3::4] = big[torch.arange(len(bias[3::4])) % len(big)]
    res = torch.randint(-32, 33, (n, cout, ho, wo), generator=g).double() / 4
    # the bound, asserted on what was generated
    assert float(x.abs().max()) <= A_MAX and float((wt * W_DEN).abs().max()) <= W_MAX and float(bias.abs().max()) <= BIAS_MAX and float(res.abs().max()) <= RES_MAX
    for t in (x, wt * W_DEN, bias * 8, res * 4):
        assert torch.equal(t, t.round())
    worst = A_MAX * W_MAX / W_DEN * cin * k * k + BIAS_MAX + RES_MAX          # the largest partial sum of any order
    assert worst * 8 < 2 ** 24, worst
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(x.to(dt).double(), x) and torch.equal(wt.to(dt).double(), wt) and torch.equal(res.to(dt).double(), res)
    assert torch.equal(bias.float().double(), bias)
    return x, wt, bias, res


def silu64(v):
    return v * torch.sigmoid(v)      # float64: -0.0 for v -> -inf side underflow, NaN for v = -inf, like the fp32 formula x / (1 + exp(-x))


@functools.lru_cache(maxsize=None)
def reference64(n, h, w, cin, cout, k, s, act, residual, seed=0):
    """float64 convolution + bias + activation + shortcut (the shortcut AFTER the activation, reference common.py:115-116), NHWC; not rounded"""
    x, wt, bias, res = exact_operands(n, h, w, cin, cout, k, s, seed)
    v = F.conv2d(x, wt, bias, s, k // 2)
    if act:
        # fp32 cannot hold exp(-v) for v < -88.7 (the 16-bit kernels and torch's fp32 SiLU both return -0 there, while the true value is a normal bf16 / fp32 number down
        # to v = -103): that edge belongs to the domain tests, which take torch's fp32 class as the reference; here no pre-activation may come near it
        assert not bool(((v < -80) & (v > -300)).any()), "a pre-activation in the band where fp32 SiLU underflows"
        v = silu64(v)
    if residual:
        v = v + res
    return v.permute(0, 2, 3, 1).contiguous()


def round_once(ref64, dtype):
    """the ONE rounding to the storage type (float64 -> fp32 is exact or far below the 16-bit spacing; fp32 -> 16 bits rounds to nearest even)"""
    return ref64.float().to(dtype)


def spacing(ref64, dtype):
    """the storage type's spacing (ulp) at |ref|, per element: 2^(max(floor(log2 |ref|), e_min) - fraction bits)"""
    _, e = torch.frexp(ref64.abs().double())        # |ref| = m * 2^e, m in [0.5, 1)  ->  floor(log2 |ref|) = e - 1 (0 -> e = 0: clamped below)
    e = torch.clamp(e.double() - 1, min=MIN_EXP[dtype])
    e = torch.where(ref64 == 0, torch.full_like(e, MIN_EXP[dtype]), e)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT_BITS[dtype])


def ulp_stats(got, ref64, dtype, scale64=None):
    """`scale64`: measure in ulps at max(|ref|, |scale|) -- for a sum whose terms cancel (fp32 SiLU + shortcut) the error of the larger term is what a kernel can be held to.
    (worst |got - round_once(ref)| in ulps, its flat index, mean signed error of got against the UNROUNDED reference in ulps -- negative = towards zero,
    number of finite elements).  Non-finite references are compared by class (NaN / +-inf) and excluded from the statistics."""
    got64 = got.double()
    want = round_once(ref64, dtype).double()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isnan(got64), torch.isnan(want)), "NaN pattern differs from the reference"
    inf_ok = torch.equal(got64[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)])
    assert inf_ok and bool(torch.isfinite(got64[fin]).all()), "+-inf pattern differs from the reference"
    if int(fin.sum()) == 0:
        return 0.0, 0, 0.0, 0
    r = torch.where(fin, ref64.double(), torch.zeros_like(want))
    g = torch.where(fin, got64, torch.zeros_like(want))
    u = spacing(r if scale64 is None else torch.maximum(r.abs(), torch.where(fin, scale64.double().abs(), torch.zeros_like(want))), dtype)
    d = ((g - torch.where(fin, want, torch.zeros_like(want))).abs() / u).reshape(-1)
    worst, idx = float(d.max()), int(d.argmax())
    sgn = torch.where(r < 0, -torch.ones_like(r), torch.ones_like(r))
    signed = ((g - r) * sgn / u)[fin]
    return worst, idx, float(signed.mean()), int(fin.sum())


def assert_elementwise(got, ref64, dtype, max_ulp, label="", note=None, scale64=None):
    """every element of `got` (storage type or fp32 tensor of the reference's shape) within `max_ulp` units of the storage type's spacing at |ref| of the once-rounded
    float64 reference; max_ulp = 0 asserts the BITS (signed zeros included).  Returns (worst ulp, mean signed ulp, elements)."""
    assert tuple(got.shape) == tuple(ref64.shape), (got.shape, ref64.shape)
    worst, idx, mean, cnt = ulp_stats(got, ref64, dtype, scale64)
    want = round_once(ref64, dtype)
    if max_ulp == 0 and got.dtype == dtype:
        bits = {2: torch.int16, 4: torch.int32}[want.element_size()]
        same = got.contiguous().view(bits) == want.contiguous().view(bits)
        nan = torch.isnan(want)
        bad = ~(same | nan)
        if bool(bad.any()):
            idx, worst = int(bad.reshape(-1).nonzero()[0]), max(worst, 0.5)   # (a signed zero of the wrong sign has distance 0)
    if worst > max_ulp:
        pos = tuple(int(i) for i in torch.unravel_index(torch.tensor(idx), ref64.shape))
        raise AssertionError(f"{label}: element {pos} (n, y, x, c) is {float(got.reshape(-1)[idx])!r}, reference {float(ref64.reshape(-1)[idx])!r} -> "
                             f"{float(want.reshape(-1)[idx])!r} once rounded: {worst:.2f} ulp > {max_ulp}; mean signed error {mean:+.3f} ulp over {cnt} elements" + ("" if note is None else note(idx)))
    return worst, mean, cnt


class Tally:
    """worst ulp and element-weighted mean signed error over the launches of one case, the mean also per GROUP of launches (the small maps / the large one: the
    (1, 17, 33) map holds nine tenths of a case's elements, and a biased path taken on the small maps alone must not hide behind it)"""

    def __init__(self):
        self.worst, self.sum, self.cnt, self.ran, self.refused, self.where, self.failures, self.groups = 0.0, 0.0, 0, 0, 0, "", [], {}

    def add(self, worst, mean, cnt, label="", group=None):
        if worst > self.worst:
            self.worst, self.where = worst, label
        self.sum += mean * cnt
        self.cnt += cnt
        self.ran += 1
        g = self.groups.setdefault(group, [0.0, 0])
        g[0] += mean * cnt
        g[1] += cnt

    def check(self, got, ref64, dtype, max_ulp, label, group=None, scale64=None):
        """assert_elementwise with the verdict deferred to `verdict()`: every launch of a case is measured and printed before anything is asserted"""
        try:
            worst, _, mean, cnt = ulp_stats(got, ref64, dtype, scale64)
            self.add(worst, mean, cnt, label, group)
            assert_elementwise(got, ref64, dtype, max_ulp, label, scale64=scale64)
        except AssertionError as e:
            self.failures.append(str(e))

    def group_means(self):
        return {g: s / max(1, c) for g, (s, c) in self.groups.items()}

    def verdict(self, label, max_mean=0.1):
        print(self.line(label))
        assert not self.failures, f"{len(self.failures)} launches of {label} fail, the first: {self.failures[0]}"
        assert abs(self.mean) <= max_mean, self.line(label)
        for g, m in self.group_means().items():
            assert abs(m) <= max_mean, f"{self.line(label)}: group {g}"

    @property
    def mean(self):
        return self.sum / max(1, self.cnt)

    def line(self, label):
        return f"EXACT {label}: {self.ran} launches ({self.refused} refused), {self.cnt} elements, worst {self.worst:.3f} ulp ({self.where}), mean signed {self.mean:+.4f} ulp" + \
               "".join(f", {g} {m:+.4f}" for g, m in self.group_means().items() if g is not None)


# ---- the activation's whole domain -------------------------------------------------------------------------------------------------
def act_domain(dtype):
    """pre-activations for the domain test, as a 1-D tensor of `dtype` (multiple of 32 long, zero padded): every finite fp16 value / every finite bf16 value
    with |v| <= 2^17, and the rows +-88, +-89, +-104 (where exp2 over / underflows in fp32)"""
    if dtype == torch.float16:
        allv = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.float16)
    else:
        allv = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    allv = allv[torch.isfinite(allv.float())]
    if dtype == torch.bfloat16:
        allv = allv[allv.float().abs() <= 2.0 ** 17]
    rows = torch.tensor([88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 0.0, -0.0], dtype=torch.float32).to(dtype)
    v = torch.cat([allv, rows])
    pad = (-len(v)) % 32
    return torch.cat([v, torch.zeros(pad, dtype=dtype)])


ACT_REFS = {
    "silu": (silu64, lambda t: F.silu(t)),
    "hardswish": (lambda v: v * torch.clamp(v + 3, 0, 6) / 6, lambda t: F.hardswish(t)),
    "leaky": (lambda v: torch.where(v >= 0, v, v * 0.1), lambda t: F.leaky_relu(t, 0.1)),
}


def assert_act_domain(got, pre64, act_name, dtype, max_ulp, label=""):
    """`got` = act(pre) as stored by the kernel.  The reference's own behaviour (torch in fp32, then .to(dtype)) decides NaN / +-0 / +-inf: the class must match; finite
    results are within `max_ulp` of the float64 activation rounded once.  Returns (worst ulp, mean signed ulp, elements)."""
    f64, f32 = ACT_REFS[act_name]
    cls = f32(pre64.float()).to(dtype)
    g = got.float()
    c = cls.float()
    assert torch.equal(torch.isnan(g), torch.isnan(c)), f"{label}: NaN pattern differs from torch's"
    assert torch.equal(torch.isinf(g), torch.isinf(c)) and torch.equal(g[torch.isinf(c)], c[torch.isinf(c)]), f"{label}: +-inf pattern differs from torch's"
    z = (c == 0)
    bad = z & ((g != 0) | (torch.signbit(g) != torch.signbit(c)))
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{label}: pre-activation {float(pre64.reshape(-1)[i])!r}: torch stores {float(c.reshape(-1)[i])!r}, the kernel {float(g.reshape(-1)[i])!r}")
    ok = torch.isfinite(c) & ~z
    ref = torch.where(ok, f64(torch.where(ok, pre64, torch.zeros_like(pre64))), torch.zeros_like(pre64))
    gg = torch.where(ok, got.double(), torch.zeros_like(pre64))
    return assert_elementwise(gg.to(dtype), ref, dtype, max_ulp, label, note=lambda i: f"; pre-activation {float(pre64.reshape(-1)[i])!r}")


def sim_cases(tile):
    """the simulator's share of cases(tile) (a lane-accurate launch costs tenths of a second): every shape and kind, one width per shape -- rotated with the tile id, so that
    a family's tiles cover all widths between them -- and every width on the small maps for the single-shape kernels (a refusal costs nothing)"""
    fam = family_of(tile) if tile not in F32_TILES else None
    _, kinds, extra = FAMILIES[fam] if fam else (None, KINDS, [])
    ws = WIDTHS + extra
    out = []
    for (k, s) in kinds:
        for i, (n, h, w) in enumerate(SHAPES):
            if fam in ("c32", "res", "rw2", "rw3", "rs"):
                out += [(n, h, w, cin, cout, k, s) for (cin, cout) in ws if (n, h, w) != SHAPES[-1] or (cin, cout) == ws[-1] or fam == "c32"]
            else:
                cin, cout = ws[0] if (n, h, w) == SHAPES[-1] else ws[(i + abs(tile) + k) % len(ws)]
                out.append((n, h, w, cin, cout, k, s))
    return out


def silu_domain_problem(dtype):
    """the domain test as ONE pointwise convolution: x (pixels, 32) of `dtype`, weight (64, 32) = two stacked identities, bias (64), and the float64 pre-activations
    (pixels, 64) the launch must see.  Pixels 0 ... hold act_domain(dtype), 32 values each.  The second identity block carries two biases, so that fp16 gets the rows no
    fp16 input can express: 65504 + 15.9921875 (the largest pre-activation that still rounds to the fp16 maximum) and 65504 + 16 (the tie that rounds to +inf).  The last
    pixel holds -inf in channel 0 (SiLU(-inf) = NaN; the zero weights of the other rows turn it into NaN there as well, in the reference as in the kernel)."""
    v = act_domain(dtype).view(-1, 32)
    extra = torch.zeros(2, 32, dtype=dtype)
    if dtype == torch.float16:
        extra[0, 0] = extra[0, 1] = 65504.0
    extra[1, 0] = float("-inf")
    x = torch.cat([v, extra])
    wt = torch.cat([torch.eye(32), torch.eye(32)]).double()
    bias = torch.zeros(64, dtype=torch.float64)
    bias[32], bias[33] = 15.9921875, 16.0
    pre = x.double() @ wt.T + bias        # (0 * -inf = NaN, like the MFMA)
    return x, wt, bias, pre + 0.0         # (+ 0.0: the accumulator starts from the bias, and 0 + -0 = +0)
