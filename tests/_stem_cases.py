"""Exact-operand cases of the network's first layer (helpers, no fixtures; used by tests/test_stem_exact_gpu.py on the GPU and by tests/test_hipsim_kernels.py on the
CPU lane simulator): the 6x6 stride-2 stem in its super-pixel, planar-image and im2col forms, Focus, and stem + body.1 as one launch.

Same rule as tests/_exact.py: pixels are integers in [-3, 3] (the image range is irrelevant to the arithmetic), weights are q / 8 with |q| <= 2, the bias is a multiple of
1/8 held in fp32, K = 3 * 6 * 6 = 108 <= _exact.K_MAX -- so every partial sum of any order is a multiple of 1/8 below 2^13 and the fp32 accumulation is exact; the float64
reference rounded ONCE is the one right answer.  Output channel o < cout - 2 carries ONE non-zero weight (tap (c, ky, kx) known: a wrong tap, a swapped colour plane or
a wrong border pixel changes an exactly known multiple of 1/8), the last two are dense.  There are 108 taps, more than any cout here, so the single-tap channels rotate
with `seed`: SETS[cout] weight sets cover all 108 between them (asserted in `tap_cover`)."""
import functools

import torch
import torch.nn.functional as F

import _exact

# (n, H, W) of the image                what it reaches
SHAPES = [
    (1, 2, 2),       # one output; every tap but 4 is padding (canvas only)
    (1, 2, 8),       # the smallest planar image (W % 8 == 0): ho 1, wo 4
    (1, 12, 2),      # a one-column output map (canvas only)
    (2, 7, 10),      # odd height, W % 8 != 0 (canvas only: the planar entry points must refuse it)
    (2, 7, 16),      # odd height, planar; stem 3x8, body.1 2x4
    (3, 18, 72),     # stem 9x36: the 8x32 stem tile ragged in both directions; body.1 5x18: the 8x16 fused tile ragged
    (1, 34, 136),    # stem 17x68: 3x3 stem tiles, the last tile row holds one row; body.1 9x34
    (1, 66, 40),     # a tall map: three fused tile rows
]
LARGE = SHAPES[-2:]
COUTS = [16, 32, 48, 64]
SETS = {16: 8, 32: 4, 48: 3, 64: 2}      # weight sets per cout: ceil(108 / (cout - 2))
NTAPS = 108


def planar_ok(shape):
    return shape[2] % 8 == 0


def group_of(shape):
    return "large maps" if tuple(shape) in LARGE else "small maps"


def stem_hw(h, w):
    """output size of Conv(3, c, 6, 2, 2)"""
    return (h + 4 - 6) // 2 + 1, (w + 4 - 6) // 2 + 1


def body1_hw(hs, ws):
    """output size of Conv(32, 64, 3, 2, 1) over the stem's map"""
    return (hs - 1) // 2 + 1, (ws - 1) // 2 + 1


def single_tap(cout, seed, o):
    """(flat tap index, q) of single-tap channel o of weight set `seed`"""
    return (seed * (cout - 2) + o) % NTAPS, (1, -2, 2)[o % 3] * (1 if (o // 3) % 2 == 0 else -1)


def tap_cover(pairs):
    """the set of taps the single-tap channels of the (cout, seed) pairs reach"""
    return {single_tap(cout, seed, o)[0] for (cout, seed) in pairs for o in range(cout - 2)}


for _c, _s in SETS.items():
    assert tap_cover([(_c, s) for s in range(_s)]) == set(range(NTAPS)), _c


def _weights(cout, seed, g, tap_shape):
    """(cout, *tap_shape) float64 weights q / 8: single-tap channels, the last two dense; tap t is the flat index into tap_shape"""
    q = torch.randint(-_exact.W_MAX, _exact.W_MAX + 1, (cout, NTAPS), generator=g)
    q[:cout - 2] = 0
    for o in range(cout - 2):
        t, v = single_tap(cout, seed, o)
        q[o, t] = v
    return q.view(cout, *tap_shape).double() / _exact.W_DEN


def _bias(cout, g):
    bias = torch.randint(-16, 17, (cout,), generator=g).double() / 8
    big = torch.tensor([1000.125, -2049.625, 33.125, -515.625, 4095.875, -1027.375], dtype=torch.float64)   # the large values of _exact (negative ones far below -88.7)
    bias[3::4] = big[torch.arange(len(bias[3::4])) % len(big)]
    return bias


def _assert_bound(x, wt, bias, k):
    assert k <= _exact.K_MAX
    assert float(x.abs().max()) <= _exact.A_MAX and float((wt * _exact.W_DEN).abs().max()) <= _exact.W_MAX and float(bias.abs().max()) <= _exact.BIAS_MAX
    for t in (x, wt * _exact.W_DEN, bias * 8):
        assert torch.equal(t, t.round())
    worst = _exact.A_MAX * _exact.W_MAX / _exact.W_DEN * k + _exact.BIAS_MAX          # the largest partial sum of any order
    assert worst * 8 < 2 ** 24, worst
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(x.to(dt).double(), x) and torch.equal(wt.to(dt).double(), wt)
    assert torch.equal(bias.float().double(), bias)


@functools.lru_cache(maxsize=None)
def stem_operands(n, h, w, cout, seed=0):
    """x (n, 3, h, w), weight (cout, 3, 6, 6), bias (cout): float64 tensors (shared: do not modify) every storage type holds exactly; tap t = (c * 6 + ky) * 6 + kx"""
    g = torch.Generator().manual_seed(1000 * seed + 13 * cout + 7 * h + 3 * w + n)
    x = torch.randint(-_exact.A_MAX, _exact.A_MAX + 1, (n, 3, h, w), generator=g).double()
    wt = _weights(cout, seed, g, (3, 6, 6))
    bias = _bias(cout, g)
    _assert_bound(x, wt, bias, 108)
    return x, wt, bias


def _finish(v, act):
    if act:
        assert not bool(((v < -80) & (v > -300)).any()), "a pre-activation in the band where fp32 SiLU underflows"
        # not vacuous: at least half of the outputs sit on the curved part of SiLU
        assert float((v.abs() <= 8).double().mean()) >= 0.5, float((v.abs() <= 8).double().mean())
        v = _exact.silu64(v)
    return v.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def stem_reference64(n, h, w, cout, seed=0, act=False):
    """float64 F.conv2d(x, w, b, 2, 2) (+ SiLU), NHWC, not rounded"""
    x, wt, bias = stem_operands(n, h, w, cout, seed)
    return _finish(F.conv2d(x, wt, bias, 2, 2), act)


def focus_transform64(x):
    """the reference's rearrangement (yolort/v5/models/common.py Focus.forward), restated: slots (0,0) (1,0) (0,1) (1,1)"""
    return torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)


@functools.lru_cache(maxsize=None)
def focus_operands(n, h, w, cout, seed=0):
    """x (n, 3, h, w), the 3x3 weight over the 12 rearranged channels (cout, 12, 3, 3), bias: tap t = (c12 * 3 + ky) * 3 + kx, 108 of them again"""
    g = torch.Generator().manual_seed(5000 + 1000 * seed + 13 * cout + 7 * h + 3 * w + n)
    x = torch.randint(-_exact.A_MAX, _exact.A_MAX + 1, (n, 3, h, w), generator=g).double()
    wt = _weights(cout, seed, g, (12, 3, 3))
    bias = _bias(cout, g)
    _assert_bound(x, wt, bias, 108)
    return x, wt, bias


@functools.lru_cache(maxsize=None)
def focus_pre64(n, h, w, cout, seed=0):
    """the REFERENCE FORMULATION in float64: Conv(12, c, 3, 1, 1) over focus_transform(x) -- not the 6x6 form; NCHW pre-activations"""
    x, wt, bias = focus_operands(n, h, w, cout, seed)
    return F.conv2d(focus_transform64(x), wt, bias, 1, 1)


# ---- stem + body.1 -----------------------------------------------------------------------------------------------------------------
def _body1_weights(g):
    """Conv(32, 64, 3, 2, 1): q / 8; the 27 single-tap channels of _exact (tap o // 3 of input channel {0, 16, 31}[o % 3]), then channels of at most 4 taps; small biases"""
    q = torch.zeros(64, 32, 3, 3, dtype=torch.int64)
    for o in range(27):
        tap, ci = o // 3, (0, 16, 31)[o % 3]
        q[o, ci, tap // 3, tap % 3] = (1, -2, 2)[o % 3] * (1 if (o // 3) % 2 == 0 else -1)
    pos = torch.randint(0, 288, (64, 4), generator=g)
    val = torch.randint(-_exact.W_MAX, _exact.W_MAX + 1, (64, 4), generator=g)
    flat = q.view(64, 288)
    for o in range(27, 64):
        for j in range(4):
            flat[o, int(pos[o, j])] = int(val[o, j])
    bias = torch.randint(-16, 17, (64,), generator=g).double() / 8
    return q.double() / _exact.W_DEN, bias


@functools.lru_cache(maxsize=None)
def body1_weights(seed=0):
    return _body1_weights(torch.Generator().manual_seed(777 + seed))


@functools.lru_cache(maxsize=None)
def two_layer_operands(n, h, w, seed=0):
    """the problem whose INTERMEDIATE is exact through SiLU: integer pixels in [-3, 3], at most 7 weights of +-1 per stem channel, stem bias 40 -> every stem
    pre-activation is an integer v in [19, 61], where v - SiLU(v) <= 1.8e-6 is far inside half an ulp of fp16 and bf16 (float64 SiLU of every integer in [16, 64) rounds to
    itself in both: asserted below), so the stored intermediate is v exactly.  body.1 pads with 0, not 40: a fused kernel that does not zero the stem pixels outside the
    stem's output is off by a known multiple of 40 / 8 at every border pixel.  body.1's accumulation is exact: 61 * 1/4 * 288 * 8 < 2^24.
    -> x (n, 3, h, w), w0 (32, 3, 6, 6), b0 (32), w1 (64, 32, 3, 3), b1 (64)"""
    g = torch.Generator().manual_seed(9000 + 1000 * seed + 7 * h + 3 * w + n)
    x = torch.randint(-_exact.A_MAX, _exact.A_MAX + 1, (n, 3, h, w), generator=g).double()
    w0 = torch.zeros(32, NTAPS, dtype=torch.float64)
    pos = torch.randint(0, NTAPS, (32, 7), generator=g)
    sgn = torch.randint(0, 2, (32, 7), generator=g).double() * 2 - 1
    for o in range(32):
        for j in range(7):
            w0[o, int(pos[o, j])] = float(sgn[o, j])
    w0 = w0.view(32, 3, 6, 6)
    b0 = torch.full((32,), 40.0, dtype=torch.float64)
    w1, b1 = body1_weights(seed)
    assert int((w0.view(32, -1) != 0).sum(1).max()) <= 7 and float(w0.abs().max()) == 1
    assert 61 * 0.25 * 288 * 8 < 2 ** 24
    return x, w0, b0, w1, b1


_ints = torch.arange(16, 64, dtype=torch.float64)
for _dt in (torch.float16, torch.bfloat16):
    assert torch.equal(_exact.round_once(_exact.silu64(_ints), _dt).double(), _ints)


def body1_reference64(mid, w1, b1):
    """float64 Conv(32, 64, 3, 2, 1) + SiLU over the NCHW intermediate `mid`, NHWC, not rounded"""
    v = F.conv2d(mid, w1, b1, 2, 1)
    assert not bool(((v < -80) & (v > -300)).any()), "a pre-activation in the band where fp32 SiLU underflows"
    return _exact.silu64(v).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def two_layer_reference64(n, h, w, seed=0):
    x, w0, b0, w1, b1 = two_layer_operands(n, h, w, seed)
    v = F.conv2d(x, w0, b0, 2, 2)
    assert torch.equal(v, v.round()) and float(v.min()) >= 19 and float(v.max()) <= 61, (float(v.min()), float(v.max()))
    return body1_reference64(v, w1, b1)      # the stored intermediate is v itself (see two_layer_operands)


# ---- guard bands -------------------------------------------------------------------------------------------------------------------
_NAN_BITS = {2: (torch.int16, 0x7fff), 4: (torch.int32, 0x7fffffff)}


def nan_fill(t):
    it, bits = _NAN_BITS[t.element_size()]
    t.view(it).fill_(bits)
    return t


def bits(t):
    return t.contiguous().view(_NAN_BITS[t.element_size()][0])


class Guard:
    """an NHWC region (optionally a channel slice [c0, c0 + c) of pixels `cs` wide) INSIDE a larger tensor filled with NaN bit patterns, which carries its own 256-byte zero
    tail: `off` / `tail` are element offsets into `t` (engine.View(base=t, off, n, h, w, c, cs, tail) on the GPU, raw pointers on the simulator)"""

    def __init__(self, n, h, w, c, dtype, device, c0=0, cs=None, guard=72):
        cs = c if cs is None else cs
        self.n, self.h, self.w, self.c, self.cs = n, h, w, c, cs
        numel = (guard + n * h * w * cs + guard + 7) // 8 * 8
        self.t = nan_fill(torch.empty(numel + 256 // torch.empty((), dtype=dtype).element_size(), dtype=dtype, device=device))
        self.t[numel:] = 0
        self.off, self.tail = guard + c0, numel
        self.before = None

    def view(self, t=None):
        return torch.as_strided(self.t if t is None else t, (self.n, self.h, self.w, self.c), (self.h * self.w * self.cs, self.w * self.cs, self.cs, 1), self.off)

    @property
    def ptr(self):
        return self.t.data_ptr() + self.off * self.t.element_size()

    @property
    def zeros(self):
        return self.t.data_ptr() + self.tail * self.t.element_size()

    def snapshot(self):
        self.before = self.t.clone()
        return self

    def assert_untouched(self, label):
        assert torch.equal(bits(self.t), bits(self.before)), f"{label}: the buffer was written"

    def assert_only_the_view_written(self, label):
        """every guard element, every channel outside the slice and the zero tail hold what they held; the view holds no NaN"""
        want = self.before.clone()
        self.view(want).copy_(self.view())
        assert torch.equal(bits(self.t), bits(want)), f"{label}: a write outside the output view"
        assert not bool(torch.isnan(self.view()).any()), f"{label}: NaN in the output"


def canvas(x, dtype, device):
    """the NHWC4 canvas of NCHW images x (float64) as a Guard: channel 3 is 0 (the letterbox's contract)"""
    n, _, h, w = x.shape
    g = Guard(n, h, w, 4, dtype, device)
    v = torch.zeros(n, h, w, 4, dtype=dtype)
    v[..., :3] = x.permute(0, 2, 3, 1).to(dtype)
    g.view().copy_(v.to(device))
    return g.snapshot()


def planar_images(x, dtype, device, shift=0):
    """(list of (3, h, w) images carved at 16-byte-aligned offsets out of ONE NaN-filled tensor, that tensor); `shift`: element offset added to every image (2 bytes: refused)"""
    n, _, h, w = x.shape
    per, gap = 3 * h * w, 72
    assert per % 8 == 0 or shift or w % 8
    step = (per + gap + 7) // 8 * 8
    t = nan_fill(torch.empty(gap + n * step + 8, dtype=dtype, device=device))
    imgs = []
    for i in range(n):
        im = t[gap + i * step + shift: gap + i * step + shift + per].view(3, h, w)
        im.copy_(x[i].to(dtype).to(device))
        imgs.append(im)
    return imgs, t
