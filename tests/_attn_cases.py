"""Operands and yardsticks of the attention tests (tests/test_attention.py, tests/test_attention_gpu.py): the float64 soft-max attention, the operand families, and the
transformer blocks written with plain nn layers -- same constructor arguments and module tree, hence the same state_dict keys, as yolort_amd.v5's."""
import functools

import torch
from torch import nn

import _ghost


def shapes():
    """(n, H, W, heads, d): one token, four tokens, one key short of / exactly / one key past a chunk, one query past a tile, and a ragged map with two full key
    chunks, a partial one and three query tiles; n in {1, 3}, heads in {1, 4} and every d between them"""
    from yolort_amd._lib import ATTN_TILE
    tq, tk = ATTN_TILE
    return [(1, 1, 1, 1, 32), (3, 2, 2, 4, 32), (1, 1, tk - 1, 1, 64), (1, 1, tk, 4, 32), (3, 1, tk + 1, 1, 128), (1, 1, tq + 1, 4, 64), (1, 10, 15, 4, 64), (3, 10, 15, 1, 128)]


def reference64(q, k, v, heads, scale):
    """softmax(scale * q k^T) v per image and head in float64; q, k, v (n, S, c)"""
    n, s, c = q.shape
    qh, kh, vh = (t.double().reshape(n, s, heads, c // heads).transpose(1, 2) for t in (q, k, v))
    return (torch.softmax(scale * qh @ kh.transpose(2, 3), -1) @ vh).transpose(1, 2).reshape(n, s, c)


@functools.lru_cache(maxsize=None)
def operands(kind, n, s, heads, d):
    """float64 q, k, v (n, S, heads * d) whose values both storage types hold exactly (shared: do not modify), and for "select" the key each query picks.
    select:  k[j] = +-1 codes (bit b of j is the sign of dimension b), q[i] = 256 k[perm(i)] with a permutation per (image, head), v non-zero integers in [-3, 3]
    uniform: q = 0, v integers;   general: q, k multiples of 9/64 in [-2.25, 2.25] -> scaled scores within about +-8 (4.5 sigma), v multiples of 1/16 in [-4, 4]"""
    g = torch.Generator().manual_seed(1000 * s + 10 * d + heads + n)
    shape = (n, s, heads, d)
    if kind == "general":
        q, k = (torch.randint(-16, 17, shape, generator=g).double() * 9 / 64 for _ in range(2))      # variance 1.8 each: d^-0.5 q . k has sigma 1.8 whatever d is
        return q.reshape(n, s, -1), k.reshape(n, s, -1), (torch.randint(-64, 65, shape, generator=g).double() / 16).reshape(n, s, -1), None
    v = torch.randint(1, 4, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    j = torch.arange(s)
    codes = torch.ones(s, d, dtype=torch.float64)
    for b in range(8):
        codes[:, b] = 1 - 2 * ((j >> b) & 1)
    k = codes[None, :, None, :].expand(shape).contiguous()
    perm = torch.stack([torch.stack([torch.randperm(s, generator=g) for _ in range(heads)], 1) for _ in range(n)])      # (n, S, heads)
    q = 256 * codes[perm] if kind == "select" else torch.zeros(shape, dtype=torch.float64)
    return q.reshape(n, s, -1), k.reshape(n, s, -1), v.reshape(n, s, -1), perm


class TransformerLayer(nn.Module):
    def __init__(self, c, num_heads):
        super().__init__()
        self.q, self.k, self.v = (nn.Linear(c, c, bias=False) for _ in range(3))
        self.ma = nn.MultiheadAttention(c, num_heads)
        self.fc1, self.fc2 = nn.Linear(c, c, bias=False), nn.Linear(c, c, bias=False)

    def forward(self, x):      # (S, b, c)
        x = self.ma(self.q(x), self.k(x), self.v(x))[0] + x
        return self.fc2(self.fc1(x)) + x


class TransformerBlock(nn.Module):
    def __init__(self, c1, c2, num_heads, num_layers):
        super().__init__()
        self.conv = _ghost.Conv(c1, c2) if c1 != c2 else None
        self.linear = nn.Linear(c2, c2)
        self.tr = nn.Sequential(*[TransformerLayer(c2, num_heads) for _ in range(num_layers)])

    def forward(self, x):      # (b, c, h, w)
        x = x if self.conv is None else self.conv(x)
        b, c, h, w = x.shape
        p = x.flatten(2).permute(2, 0, 1)
        return self.tr(p + self.linear(p)).permute(1, 2, 0).reshape(b, c, h, w)


class C3TR(nn.Module):
    def __init__(self, c1, c2, n=1):
        super().__init__()
        self.cv1, self.cv2, self.cv3 = _ghost.Conv(c1, c2 // 2), _ghost.Conv(c1, c2 // 2), _ghost.Conv(c2, c2)
        self.m = TransformerBlock(c2 // 2, c2 // 2, 4, n)

    def forward(self, x):
        return self.cv3(torch.cat([self.m(self.cv1(x)), self.cv2(x)], 1))


# constructor arguments.  C3TR has four heads of c2 / 8 channels, so 256 is the narrowest c2 the kernel's head dimensions (32, 64, 128) admit: C3TR(64, 64) is refused
CASES = {"TransformerLayer": (64, 2), "TransformerBlock": (32, 64, 2, 2), "C3TR": (64, 256, 1)}


def pair(name):
    """(yolort_amd.v5 module, nn twin) of a case, both in eval mode"""
    import yolort_amd.v5 as V
    return getattr(V, name)(*CASES[name]).eval(), globals()[name](*CASES[name]).eval()
