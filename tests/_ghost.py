"""The depthwise family written with plain nn layers: same constructor arguments and module tree -- hence the same state_dict keys -- as yolort_amd.v5's DWConv /
GhostConv / GhostBottleneck / C3Ghost; evaluated in float64 it is the yardstick of the block tests (tests/test_dwconv.py, tests/test_dwconv_gpu.py)."""
import torch
from torch import nn


class Conv(nn.Module):
    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, k // 2, groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2, eps=1e-3)
        self.act = nn.SiLU() if act else nn.Identity()

    def forward(self, x):
        return self.act(self.bn(self.conv(x)))


def DWConv(c1, c2, k=1, s=1, act=True):
    return Conv(c1, c2, k, s, c1, act)


class GhostConv(nn.Module):
    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        self.cv1, self.cv2 = Conv(c1, c2 // 2, k, s, g, act), Conv(c2 // 2, c2 // 2, 5, 1, c2 // 2, act)

    def forward(self, x):
        return torch.cat([self.cv1(x), self.cv2(self.cv1(x))], 1)


class GhostBottleneck(nn.Module):
    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        self.conv = nn.Sequential(GhostConv(c1, c2 // 2), DWConv(c2 // 2, c2 // 2, k, s, False) if s == 2 else nn.Identity(), GhostConv(c2 // 2, c2, act=False))
        self.shortcut = nn.Sequential(DWConv(c1, c1, k, s, False), Conv(c1, c2, act=False)) if s == 2 else nn.Identity()

    def forward(self, x):
        return self.conv(x) + self.shortcut(x)


class C3Ghost(nn.Module):
    def __init__(self, c1, c2, n=1):
        super().__init__()
        self.cv1, self.cv2, self.cv3 = Conv(c1, c2 // 2), Conv(c1, c2 // 2), Conv(c2, c2)
        self.m = nn.Sequential(*[GhostBottleneck(c2 // 2, c2 // 2) for _ in range(n)])

    def forward(self, x):
        return self.cv3(torch.cat([self.m(self.cv1(x)), self.cv2(x)], 1))


CASES = {"DWConv": (64, 64, 3, 2), "GhostConv": (64, 64), "GhostBottleneck.s1": (64, 64, 3, 1), "GhostBottleneck.s2": (64, 128, 3, 2), "C3Ghost": (64, 64, 2)}   # constructor arguments


def pair(name):
    """(yolort_amd.v5 module, nn twin) of a case, both in eval mode"""
    import yolort_amd.v5 as V
    kind = name.split(".")[0]
    return getattr(V, kind)(*CASES[name]).eval(), globals()[kind](*CASES[name]).eval()
