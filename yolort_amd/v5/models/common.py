"""YOLOv5 building blocks (r3.1 / r4.0 / r6.0 forms) as HIP plan emitters.

Same constructor signatures, attribute names and state_dict keys as the reference's blocks
(yolort/v5/models/common.py: Conv :42, DWConv :76, Bottleneck :94, BottleneckCSP :119, C3 :149, SPP :176, SPPF :190, Focus :210, C3Ghost :378, GhostConv :386,
GhostBottleneck :399, TransformerLayer :308, TransformerBlock :334, C3TR :362) so that its
checkpoints load unchanged; the arithmetic is the fused implicit-GEMM kernel (csrc/conv_igemm.hip)
instead of conv2d -> BatchNorm2d -> SiLU -> cat, and the depthwise kernel (csrc/dwconv.hip) for the convolutions with groups == channels, and the
attention kernel (csrc/attention.hip) for nn.MultiheadAttention.
"""
from __future__ import annotations

import math
import os

from typing import Dict, Optional, Tuple

import torch
from torch import nn

from ..._lib import ACT_HARDSWISH, ACT_LEAKY, ACT_NONE, ACT_SILU, YmiError
from ...engine import PackedConv, PackedConvI8, PackedDWConv, Plan, View, fold_linear
from ...hipmodule import HipModule, view_to_nchw as _view_to_nchw

__all__ = ["Conv", "DWConv", "QConv", "Bottleneck", "BottleneckCSP", "C3", "C3Ghost", "GhostConv", "GhostBottleneck", "SPP", "SPPF", "Focus", "Classify", "TransformerLayer", "TransformerBlock",
           "C3TR", "autopad", "focus_transform", "space_to_depth"]

BN_EPS, BN_MOMENTUM = 1e-3, 0.03  # set after construction by the reference (darknetv6.py:110-112)


def autopad(k, p=None):
    """'same' padding (reference common.py:35-39)."""
    if p is None:
        p = k // 2 if isinstance(k, int) else [x // 2 for x in k]
    return p


def act_code(act: nn.Module) -> int:
    """the epilogue's activation code (include/yolort_amd.h YMI_ACT_*) of the activation modules the reference's blocks use"""
    if isinstance(act, nn.SiLU):
        return ACT_SILU
    if isinstance(act, nn.Identity):
        return ACT_NONE
    if isinstance(act, nn.Hardswish):
        return ACT_HARDSWISH
    if isinstance(act, nn.LeakyReLU) and abs(act.negative_slope - 0.1) < 1e-12:
        return ACT_LEAKY
    raise NotImplementedError(f"activation {act!r} is not fused (SiLU, Hardswish, LeakyReLU(0.1) and identity are)")


class Conv(HipModule):
    """conv2d (no bias) + BatchNorm2d + SiLU (r4.0 / r6.0) or Hardswish (r3.1), fused (reference common.py:42-73).  g == c1 == c2 is the depthwise form
    (csrc/dwconv.hip: k in {3, 5}, s in {1, 2}, 'same' padding, every activation in its epilogue); any other g != 1 is not implemented."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True, version="r4.0"):
        super().__init__()
        if g != 1 and not (g == c1 == c2):
            raise NotImplementedError("grouped convolutions are not on the YOLOv5 hot path")
        if g != 1 and (k not in (3, 5) or s not in (1, 2) or autopad(k, p) != k // 2):
            raise NotImplementedError(f"the depthwise kernel implements k in {{3, 5}}, s in {{1, 2}} and padding k // 2 (got k = {k}, s = {s}, p = {p})")
        if version not in ("r4.0", "r3.1"):
            raise NotImplementedError(f"Currently doesn't support version {version}.")
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2, eps=BN_EPS, momentum=BN_MOMENTUM)
        default = nn.SiLU() if version == "r4.0" else nn.Hardswish()   # reference :62-65
        self.act = default if act is True else (act if isinstance(act, nn.Module) else nn.Identity())
        act_code(self.act)   # refuses activations that no epilogue carries
        self._packed: Dict[Tuple, Tuple] = {}

    def _is_stem(self) -> bool:
        return self.conv.in_channels == 3 and self.conv.kernel_size == (6, 6) and self.conv.stride == (2, 2) and self.conv.padding == (2, 2)

    def _input_cpad(self, c: int) -> int:
        return 4 if self._is_stem() else (c + 7) // 8 * 8

    @property
    def depthwise(self) -> bool:
        return self.conv.groups != 1

    def packed(self, dtype: torch.dtype, device: torch.device, cin_view: int):
        sig = tuple(t._version for t in (self.conv.weight, self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var)) + (self.conv.weight.data_ptr(),)
        stem = cin_view == 4 and self._is_stem()
        key = (dtype, device, cin_view, stem)
        hit = self._packed.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        bn = (self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var, float(self.bn.eps))
        pc = PackedDWConv(self.conv.weight, None, bn, dtype, device) if self.depthwise else PackedConv(self.conv.weight, None, bn, dtype, device, cin_pad=None if stem else cin_view, stem_superpixel=stem)
        self._packed[key] = (sig, pc)
        return pc

    def emit(self, plan: Plan, x: View, out: Optional[View] = None, res: Optional[View] = None, name: str = "conv", up2_out: Optional[View] = None,
             chain=None) -> View:
        pc = self.packed(plan.dtype, plan.device, x.c)
        if self.depthwise:
            if up2_out is not None or chain is not None:
                raise YmiError(f"{name}: a depthwise convolution carries no folded upsample and no chained convolution")
            return plan.dwconv(x, pc, self.conv.kernel_size[0], self.conv.stride[0], act_code(self.act), out=out, res=res, name=name)
        return plan.conv(x, pc, self.conv.stride, self.conv.padding, act_code(self.act), out=out, res=res, name=name, up2_out=up2_out, chain=chain)


class DWConv(Conv):
    """Depthwise Conv (reference common.py:76-91: groups = gcd(c1, c2)).  Implemented where c1 == c2 (pure depthwise, no channel multiplier) and k is 3 or 5."""

    def __init__(self, c1, c2, k=1, s=1, act=True, version="r4.0"):
        if c1 != c2 or k not in (3, 5):
            raise NotImplementedError(f"DWConv is implemented for c1 == c2 (no channel multiplier, no partial groups) and k in {{3, 5}}, got c1 = {c1}, c2 = {c2}, k = {k}")
        super().__init__(c1, c2, k, s, g=math.gcd(c1, c2), act=act, version=version)


class QConv(HipModule):
    """A Conv quantised after training: int8 activations and weights on the i8 matrix instruction, the folded BatchNorm, the activation, the shortcut and the
    requantisation in the epilogue (ymi_conv2d_i8, csrc/conv_i8.hip).  Built with QConv.from_float(conv, in_scale, out_scale) from an eval-mode Conv: symmetric
    per-output-channel weight scales (engine.PackedConvI8), one scale for the input tensor and one for the output.  With `out_scale` the block emits int8, so chains of
    QConv stay in the integer domain; with out_scale = None it emits the plan's 16-bit dtype and ends the chain.  g == 1, k in {1, 3}, stride in {1, 2}; anything else
    raises NotImplementedError.  The state_dict holds wq (int8 OIHW), w_scale, bias, in_scale and out_scale (0 = none) as buffers.  Picking the scales
    (calibration) is the caller's business."""

    def __init__(self, c1, c2, k=1, s=1, act=ACT_SILU):
        super().__init__()
        if k not in (1, 3) or s not in (1, 2):
            raise NotImplementedError(f"the int8 kernel implements k in {{1, 3}}, s in {{1, 2}} and padding k // 2 (got k = {k}, s = {s})")
        if c1 % 16 or c2 % 8:
            raise NotImplementedError(f"the int8 kernel needs c1 % 16 == 0 and c2 % 8 == 0 (got {c1} -> {c2})")
        self.k, self.s, self.act_code = k, s, act
        self.register_buffer("wq", torch.zeros(c2, c1, k, k, dtype=torch.int8))
        self.register_buffer("w_scale", torch.ones(c2, dtype=torch.float64))
        self.register_buffer("bias", torch.zeros(c2, dtype=torch.float32))
        self.register_buffer("in_scale", torch.ones((), dtype=torch.float64))
        self.register_buffer("out_scale", torch.zeros((), dtype=torch.float64))
        self._packed: Dict[Tuple, Tuple] = {}

    @classmethod
    def from_float(cls, conv: Conv, in_scale: float, out_scale: Optional[float] = None) -> "QConv":
        if not isinstance(conv, Conv) or conv.training:
            raise NotImplementedError("QConv.from_float takes a Conv in eval mode (BatchNorm is folded from its running statistics)")
        c = conv.conv
        k, s = c.kernel_size[0], c.stride[0]
        if c.groups != 1 or c.kernel_size != (k, k) or c.stride != (s, s) or c.padding != (k // 2, k // 2):
            raise NotImplementedError(f"the int8 kernel implements g = 1, square k in {{1, 3}} and padding k // 2 (got g = {c.groups}, k = {c.kernel_size}, p = {c.padding})")
        q = cls(c.in_channels, c.out_channels, k, s, act_code(conv.act))
        bn = (conv.bn.weight, conv.bn.bias, conv.bn.running_mean, conv.bn.running_var, float(conv.bn.eps))
        pc = PackedConvI8(c.weight, None, bn, in_scale, torch.device("cpu"))
        q.wq.copy_(pc.wq)
        q.w_scale.copy_(pc.w_scale)
        q.bias.copy_(pc.bias)
        q.in_scale.fill_(float(in_scale))
        q.out_scale.fill_(0.0 if out_scale is None else float(out_scale))
        return q.to(c.weight.device).eval()

    def packed(self, device: torch.device) -> PackedConvI8:
        sig = tuple(t._version for t in (self.wq, self.w_scale, self.bias, self.in_scale)) + (self.wq.data_ptr(),)
        hit = self._packed.get(device)
        if hit is not None and hit[0] == sig:
            return hit[1]
        pc = PackedConvI8.from_quantized(self.wq, self.w_scale, self.bias, float(self.in_scale), device)
        self._packed[device] = (sig, pc)
        return pc

    def emit(self, plan: Plan, x: View, out: Optional[View] = None, res: Optional[View] = None, res_scale: float = 1.0, name: str = "qconv") -> View:
        """`x`: an int8 view (codes of value / in_scale); a 16-bit view -- the edge of forward() -- is quantised with in_scale first"""
        if x.dtype != torch.int8:
            x = plan.quantize_i8(x, float(self.in_scale), name=name + ".quantize")
        osc = float(self.out_scale)
        return plan.conv_i8(x, self.packed(plan.device), self.s, self.act_code, out_scale=osc if osc > 0.0 else None, out=out, res=res, res_scale=res_scale, name=name)

    def _forward_on_device(self, xs, is_list):
        y = self._run_plan(xs, is_list)
        if y.dtype == torch.int8:   # the codes, NCHW
            return y.as_tensor().permute(0, 3, 1, 2).contiguous()
        return _view_to_nchw(y, xs[0].dtype)


class GhostConv(HipModule):
    """cat(cv1(x), cv2(cv1(x))), cv2 a depthwise 5 x 5 (reference common.py:386-396).  No concat kernel: cv1 writes channels [0, c_) of the c2-channel output, the
    depthwise launch reads that slice (pixel stride c2) and writes [c_, 2 c_).  Two launches.
    `res` (GhostBottleneck's sum): the depthwise half takes its half of the shortcut in its epilogue.  The first half is both the depthwise convolution's input
    (without the shortcut, read as halo by other workgroups) and the block's output (with it), so it cannot be updated by that launch: a third launch runs cv1 again
    with the shortcut in ITS epilogue and overwrites the half -- the traffic of an in-place add (read c_, read c_, write c_ channels), one rounding instead of two."""

    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = Conv(c1, c_, k, s, None, g, act)
        self.cv2 = Conv(c_, c_, 5, 1, None, c_, act)

    def emit(self, plan: Plan, x: View, out: Optional[View] = None, res: Optional[View] = None, name: str = "ghostconv") -> View:
        c_ = self.cv1.conv.out_channels
        if c_ % 8:
            raise YmiError(f"{name}: GhostConv's half width {c_} must be a multiple of 8")
        if out is None:
            k, s, p = self.cv1.conv.kernel_size[0], self.cv1.conv.stride[0], self.cv1.conv.padding[0]
            out = plan.alloc(x.n, (x.h + 2 * p - k) // s + 1, (x.w + 2 * p - k) // s + 1, 2 * c_)
        if out.c != 2 * c_ or (res is not None and res.c != 2 * c_):
            raise YmiError(f"{name}: output / shortcut views must have {2 * c_} channels")
        y = self.cv1.emit(plan, x, out=out.slice_c(0, c_), name=name + ".cv1")
        self.cv2.emit(plan, y, out=out.slice_c(c_, c_), res=None if res is None else res.slice_c(c_, c_), name=name + ".cv2")
        if res is not None:
            self.cv1.emit(plan, x, out=out.slice_c(0, c_), res=res.slice_c(0, c_), name=name + ".cv1+res")
        return out


class GhostBottleneck(HipModule):
    """conv(x) + shortcut(x) (reference common.py:399-416), conv = GhostConv, (DWConv s2), GhostConv without activation.  The sum costs no pass over the whole output:
    it rides in the last GhostConv's epilogues (see GhostConv.emit).  Launches: s == 1 (shortcut = x, needs c1 == c2): 2 + 3 = 5;  s == 2: the shortcut branch first
    (DWConv s2, 1x1 Conv: 2), then 2 + 1 + 3: 8 in all."""

    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        c_ = c2 // 2
        self.conv = nn.Sequential(GhostConv(c1, c_, 1, 1), DWConv(c_, c_, k, s, act=False) if s == 2 else nn.Identity(), GhostConv(c_, c2, 1, 1, act=False))
        self.shortcut = nn.Sequential(DWConv(c1, c1, k, s, act=False), Conv(c1, c2, 1, 1, act=False)) if s == 2 else nn.Identity()

    def emit(self, plan: Plan, x: View, out: Optional[View] = None, name: str = "ghostbottleneck") -> View:
        if isinstance(self.shortcut, nn.Identity):
            if x.c != 2 * self.conv[2].cv1.conv.out_channels:
                raise YmiError(f"{name}: the identity shortcut needs c1 == c2")
            res = x
        else:
            res = self.shortcut[1].emit(plan, self.shortcut[0].emit(plan, x, name=name + ".shortcut.0"), name=name + ".shortcut.1")
        y = self.conv[0].emit(plan, x, name=name + ".conv.0")
        if not isinstance(self.conv[1], nn.Identity):
            y = self.conv[1].emit(plan, y, name=name + ".conv.1")
        return self.conv[2].emit(plan, y, out=out, res=res, name=name + ".conv.2")


class Bottleneck(HipModule):
    """x + cv2(cv1(x)) (1x1 then 3x3); the residual add rides in cv2's epilogue (reference :94-116)."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5, version="r4.0"):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1, version=version)
        self.cv2 = Conv(c_, c2, 3, 1, g=g, version=version)
        self.add = shortcut and c1 == c2

    def emit(self, plan: Plan, x: View, out: Optional[View] = None, name: str = "bottleneck", t: Optional[View] = None, chain=None, chain_name: Optional[str] = None) -> View:
        """`t`: cv1's output when the producer of x already computed it (chained 1x1, see C3.emit);
        `chain`: a conv chained to cv2's output (C3.cv3 over the concat), passed through to Plan.conv"""
        if t is not None:
            y = t
        else:
            c_ = self.cv1.conv.out_channels
            # a hidden width that is not a multiple of 32 (yolov5m: 48 at 320 x 320) would send the 3x3 through the im2col-TABLE form of the
            # implicit GEMM (k32 operand chunks straddle taps: 0.13 of its bound, profiles/r02z_layer_table_c3.csv).  Instead cv1 writes its
            # c_ channels into a zero-initialised buffer of round_up(c_, 32) channels and the 3x3 reads all of them against weights whose
            # extra K rows are zero: the unit-tap kernels (LDS halo, resident weights) apply, for a third more bytes on this one tensor.
            cp = (c_ + 31) // 32 * 32
            if cp != c_ and c_ > 32 and not plan.fp32 and os.environ.get("YOLORT_AMD_PAD_HIDDEN", "1") != "0" and self.cv2.conv.groups == 1:
                tb = plan.alloc(x.n, x.h, x.w, cp, zero=True)
                self.cv1.emit(plan, x, out=tb.slice_c(0, c_), name=name + ".cv1")
                y = tb
            else:
                y = self.cv1.emit(plan, x, name=name + ".cv1")
        tag = ".cv2"
        if chain is not None:
            tag = ".cv2+" + (chain_name or "cv3")
        return self.cv2.emit(plan, y, out=out, res=x if self.add else None, name=name + tag, chain=chain)


class C3(HipModule):
    """cv3(cat(m(cv1(x)), cv2(x))) (reference :149-173).  The concat buffer is allocated first; the
    last bottleneck and cv2 write straight into its two halves, so no cat kernel exists."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5, version="r4.0"):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1, version=version)
        self.cv2 = Conv(c1, c_, 1, 1, version=version)
        self.cv3 = Conv(2 * c_, c2, 1, version=version)
        self.m = nn.Sequential(*[Bottleneck(c_, c_, shortcut, g, e=1.0, version=version) for _ in range(n)])
        self._pair: Dict[Tuple, Tuple] = {}

    @property
    def out_channels(self) -> int:
        return self.cv3.conv.out_channels

    def packed_pair(self, dtype: torch.dtype, device: torch.device, cin_view: int) -> PackedConv:
        """cv1 and cv2 read the same input: their folded weights are stacked along cout so ONE launch
        computes both (the kernel's second-output feature routes cv2's half into the concat buffer)."""
        mods = (self.cv1, self.cv2)
        sig = tuple(t._version for m in mods for t in (m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var)) + (self.cv1.conv.weight.data_ptr(),)
        key = (dtype, device, cin_view)
        hit = self._pair.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        cat = lambda f: torch.cat([f(m) for m in mods])  # noqa: E731
        bn = (cat(lambda m: m.bn.weight), cat(lambda m: m.bn.bias), cat(lambda m: m.bn.running_mean), cat(lambda m: m.bn.running_var), float(self.cv1.bn.eps))
        pc = PackedConv(cat(lambda m: m.conv.weight), None, bn, dtype, device, cin_pad=cin_view)
        self._pair[key] = (sig, pc)
        return pc

    def emit(self, plan: Plan, x: View, out: Optional[View] = None, name: str = "c3") -> View:
        c_ = self.cv1.conv.out_channels
        blocks = list(self.m) if isinstance(self.m, nn.Sequential) else [self.m]   # (C3TR: `m` is one TransformerBlock)
        nb = len(blocks)
        # default (YOLORT_AMD_FUSE_C3=0 turns it off, engine.Plan.fuse_c3): the whole block in one launch when it is the instance
        # csrc/c3_fused32.hip holds -- 64 -> 64, one shortcut Bottleneck of 32 hidden channels (yolov5s backbone.body.2)
        if (getattr(plan, "fuse_c3", False) and not plan.use_v1 and nb == 1 and c_ == 32 and x.c == 64 and self.cv3.conv.out_channels == 64
                and isinstance(blocks[0], Bottleneck) and blocks[0].add and blocks[0].cv1.conv.kernel_size == (1, 1) and blocks[0].cv2.conv.kernel_size == (3, 3)
                and blocks[0].cv2.conv.groups == 1
                and all(isinstance(c.act, nn.SiLU) for c in (self.cv1, self.cv2, self.cv3, blocks[0].cv1, blocks[0].cv2))
                and (out is None or out.cs % 8 == 0) and x.cs % 8 == 0):
            b0 = blocks[0]
            return plan.c3_fused(x, self.packed_pair(plan.dtype, plan.device, x.c), b0.cv1.packed(plan.dtype, plan.device, c_),
                                 b0.cv2.packed(plan.dtype, plan.device, c_), self.cv3.packed(plan.dtype, plan.device, 2 * c_), out=out, name=name + ".fused")
        # round 6 (csrc/c3_tile.hip): hidden widths 64 / 128 on maps whose halo strip of whole rows fits the LDS patch -- the whole block in one launch, or
        # one launch per Bottleneck (HEAD, MID ..., TAIL); intermediates of a launch never reach memory, weights stream in fragment order
        if (nb >= 1 and self.cv3.conv.out_channels == 2 * c_ and getattr(plan, "c3_tile_on", False) and plan.c3_tile_ok(x, c_)
                and all(isinstance(b, Bottleneck) and b.cv1.conv.kernel_size == (1, 1) and b.cv2.conv.kernel_size == (3, 3) and b.cv2.conv.stride == (1, 1)
                        and b.cv2.conv.groups == 1 and b.cv1.conv.out_channels == c_ and b.cv2.conv.out_channels == c_ and b.add == blocks[0].add
                        and isinstance(b.cv1.act, nn.SiLU) and isinstance(b.cv2.act, nn.SiLU) for b in blocks)
                and all(isinstance(c.act, nn.SiLU) for c in (self.cv1, self.cv2, self.cv3)) and (out is None or out.cs % 8 == 0)):
            pk = lambda cv, cin: cv.packed(plan.dtype, plan.device, cin)  # noqa: E731
            pc12, pc3 = self.packed_pair(plan.dtype, plan.device, x.c), pk(self.cv3, 2 * c_)
            add = bool(blocks[0].add)
            if nb == 1:
                return plan.c3_tile(0, pk(blocks[0].cv1, c_), pk(blocks[0].cv2, c_), add, x=x, pc12=pc12, pc3=pc3, out=out, name=name + ".tile")
            y2 = plan.alloc(x.n, x.h, x.w, c_)
            ping = [plan.alloc(x.n, x.h, x.w, c_), plan.alloc(x.n, x.h, x.w, c_) if nb > 2 else None]
            cur = plan.c3_tile(1, pk(blocks[0].cv1, c_), pk(blocks[0].cv2, c_), add, x=x, pc12=pc12, y1_out=ping[0], y2=y2, name=name + ".tile.cv1+cv2+m.0")
            for j in range(1, nb - 1):
                cur = plan.c3_tile(2, pk(blocks[j].cv1, c_), pk(blocks[j].cv2, c_), add, y1_in=cur, y1_out=ping[j % 2], name=f"{name}.tile.m.{j}")
            return plan.c3_tile(3, pk(blocks[nb - 1].cv1, c_), pk(blocks[nb - 1].cv2, c_), add, y1_in=cur, y2=y2, pc3=pc3, out=out, name=f"{name}.tile.m.{nb - 1}+cv3")
        cat = plan.alloc(x.n, x.h, x.w, 2 * c_)
        fuse = (not plan.use_v1) and c_ % 8 == 0 and nb >= 1 and isinstance(self.cv1.act, nn.SiLU) and isinstance(self.cv2.act, nn.SiLU)
        t0 = None
        if fuse:
            y = plan.alloc(x.n, x.h, x.w, c_)
            b0 = blocks[0]
            # the first Bottleneck's 1x1 (cv1) rides in the same launch: its input is this conv's freshly rounded output
            chain_ok = (plan.chain_1x1 and c_ in (32, 64) and   # (K = 128 works in the kernels but costs the main conv more than the saved launch: measured in round 4, not emitted)
                         isinstance(b0, Bottleneck) and isinstance(b0.cv1.act, nn.SiLU) and b0.cv1.conv.kernel_size == (1, 1)
                        and b0.cv1.conv.out_channels % 32 == 0 and b0.cv1.conv.out_channels <= 128)
            chain = None
            if chain_ok:
                t0 = plan.alloc(x.n, x.h, x.w, b0.cv1.conv.out_channels)
                chain = (b0.cv1.packed(plan.dtype, plan.device, c_), t0)
            plan.conv(x, self.packed_pair(plan.dtype, plan.device, x.c), 1, 0, ACT_SILU, out=y, out2=cat.slice_c(c_, c_), split=c_,
                      name=name + (".cv1+cv2+m.0.cv1" if chain_ok else ".cv1+cv2"), chain=chain)
        else:
            y = self.cv1.emit(plan, x, out=cat.slice_c(0, c_) if nb == 0 else None, name=name + ".cv1")
        # cv3 over the concat [last Bottleneck output | cv2(x)] rides in the last Bottleneck's 3x3 launch: its first K range is
        # that launch's rounded output in registers, the second is read from the concat buffer's other half
        c2 = self.cv3.conv.out_channels
        chain3 = None
        if (fuse and plan.chain_1x1 and plan.chain_cv3 and nb >= 1 and c_ in (32, 64) and c2 % 32 == 0 and c2 <= 128 and isinstance(self.cv3.act, nn.SiLU)
                and isinstance(blocks[nb - 1], Bottleneck) and blocks[nb - 1].cv2.conv.kernel_size == (3, 3) and blocks[nb - 1].cv2.conv.out_channels == c_):
            o3 = out if out is not None else plan.alloc(x.n, x.h, x.w, c2)
            chain3 = (self.cv3.packed(plan.dtype, plan.device, 2 * c_), o3, cat.slice_c(c_, c_))
        t_next = None
        for j, b in enumerate(blocks):
            kw = {}
            if j == 0 and t0 is not None:
                kw["t"] = t0
            elif t_next is not None:
                kw["t"] = t_next
            t_next = None
            if j == nb - 1 and chain3 is not None:
                kw["chain"] = chain3
            elif (j < nb - 1 and getattr(plan, "chain_next", False) and (plan.chain_next is True or plan.chain_next == c_) and not plan.use_v1 and c_ in (32, 64, 128) and isinstance(b, Bottleneck) and isinstance(blocks[j + 1], Bottleneck)
                  and b.cv2.conv.kernel_size == (3, 3) and b.cv2.conv.stride == (1, 1) and b.cv2.conv.groups == 1 and b.cv2.conv.out_channels == c_
                  and isinstance(b.cv2.act, nn.SiLU) and isinstance(blocks[j + 1].cv1.act, nn.SiLU) and blocks[j + 1].cv1.conv.kernel_size == (1, 1)
                  and blocks[j + 1].cv1.conv.out_channels % 32 == 0 and blocks[j + 1].cv1.conv.out_channels <= 128):
                # this Bottleneck's 3x3 carries the next one's 1x1 in its epilogue (reference :115-116 twice: x + cv2(cv1(x)), then cv1 of the next)
                nxt = blocks[j + 1]
                t_next = plan.alloc(x.n, x.h, x.w, nxt.cv1.conv.out_channels)
                kw["chain"] = (nxt.cv1.packed(plan.dtype, plan.device, c_), t_next)
                kw["chain_name"] = f"m.{j + 1}.cv1"
            y = b.emit(plan, y, out=cat.slice_c(0, c_) if j == nb - 1 else None, name=f"{name}.m.{j}" if isinstance(self.m, nn.Sequential) else name + ".m", **kw)
        if not fuse:
            self.cv2.emit(plan, x, out=cat.slice_c(c_, c_), name=name + ".cv2")
        if chain3 is not None:
            return chain3[1]
        return self.cv3.emit(plan, cat, out=out, name=name + ".cv3")


class C3Ghost(C3):
    """C3 whose `m` holds GhostBottlenecks (reference common.py:378-383).  C3.emit's fused, strip and chained forms test isinstance(..., Bottleneck), so it takes the
    general path: cv1 + cv2 in one launch, every GhostBottleneck through its own emit, the last one writing into the concat half, cv3."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[GhostBottleneck(c_, c_) for _ in range(n)])


def _tensors_sig(*tensors) -> Tuple:
    return tuple((t._version, t.data_ptr()) for t in tensors)


class TransformerLayer(HipModule):
    """x = ma(q(x), k(x), v(x)) + x;  x = fc2(fc1(x)) + x over the pixels of a map as tokens (reference common.py:308-331; no LayerNorm).  `ma` is an
    nn.MultiheadAttention kept as the parameter holder (`ma.in_proj_weight`, `ma.in_proj_bias`, `ma.out_proj.*`): its arithmetic is four launches --
      1. qkv: ONE biased 1 x 1 convolution c -> 3c whose weight is in_proj_weight[part] @ {q, k, v}.weight and whose bias is in_proj_bias.  Two Linear maps with nothing
         between them are one Linear: the product is taken in float64 at pack time and rounded ONCE, where the reference rounds q(x) to 16 bits between the two;
      2. the attention kernel (csrc/attention.hip) on the three channel slices of that buffer, the d ** -0.5 as the kernel's `scale`;
      3. out_proj with its bias and the shortcut x in the epilogue;
      4. fc2 @ fc1 folded the same way (the reference rounds fc1's output in between), the shortcut in the epilogue.
    The fold changes which 16-bit roundings happen, not the function: the float64 evaluation of the unfolded module is the yardstick of the tests."""

    def __init__(self, c, num_heads):
        super().__init__()
        if c % num_heads or c // num_heads not in (32, 64, 128):
            raise NotImplementedError(f"the attention kernel implements head dimensions 32, 64 and 128 (got c = {c}, num_heads = {num_heads})")
        self.q = nn.Linear(c, c, bias=False)
        self.k = nn.Linear(c, c, bias=False)
        self.v = nn.Linear(c, c, bias=False)
        self.ma = nn.MultiheadAttention(embed_dim=c, num_heads=num_heads)
        self.fc1 = nn.Linear(c, c, bias=False)
        self.fc2 = nn.Linear(c, c, bias=False)
        self._packed: Dict[Tuple, Tuple] = {}

    def packed(self, dtype: torch.dtype, device: torch.device) -> Tuple[PackedConv, PackedConv, PackedConv]:
        """(qkv, out_proj, fc2 @ fc1) as biased 1 x 1 convolutions"""
        ma = self.ma
        sig = _tensors_sig(self.q.weight, self.k.weight, self.v.weight, ma.in_proj_weight, ma.in_proj_bias, ma.out_proj.weight, ma.out_proj.bias, self.fc1.weight, self.fc2.weight)
        hit = self._packed.get((dtype, device))
        if hit is not None and hit[0] == sig:
            return hit[1]
        wq, wk, wv = ma.in_proj_weight.chunk(3)
        pcs = (fold_linear([(self.q.weight, wq), (self.k.weight, wk), (self.v.weight, wv)], ma.in_proj_bias, dtype, device),
               fold_linear([(ma.out_proj.weight,)], ma.out_proj.bias, dtype, device), fold_linear([(self.fc1.weight, self.fc2.weight)], None, dtype, device))
        self._packed[(dtype, device)] = (sig, pcs)
        return pcs

    def emit(self, plan: Plan, x: View, out: Optional[View] = None, name: str = "transformerlayer") -> View:
        c = self.q.in_features
        if x.c != c:
            raise YmiError(f"{name}: input view has {x.c} channels, the layer expects {c}")
        pc_qkv, pc_out, pc_fc = self.packed(plan.dtype, plan.device)
        qkv = plan.conv(x, pc_qkv, 1, 0, ACT_NONE, name=name + ".qkv")
        a = plan.attention(qkv.slice_c(0, c), qkv.slice_c(c, c), qkv.slice_c(2 * c, c), self.ma.num_heads, name=name + ".ma")
        y = plan.conv(a, pc_out, 1, 0, ACT_NONE, res=x, name=name + ".ma.out_proj")
        return plan.conv(y, pc_fc, 1, 0, ACT_NONE, out=out, res=y, name=name + ".fc1+fc2")


class TransformerBlock(HipModule):
    """tr(p + linear(p)) on the c2-channel map, after a Conv(c1, c2) when c1 != c2 (reference common.py:334-359).  The reference's flatten / transpose to (S, b, c)
    tokens is the NHWC view itself: `linear` (the learnable position embedding) is a biased 1 x 1 convolution with the shortcut in its epilogue, then the layers."""

    def __init__(self, c1, c2, num_heads, num_layers):
        super().__init__()
        self.conv = None
        if c1 != c2:
            self.conv = Conv(c1, c2)
        self.linear = nn.Linear(c2, c2)
        self.tr = nn.Sequential(*[TransformerLayer(c2, num_heads) for _ in range(num_layers)])
        self.c2 = c2
        self._packed: Dict[Tuple, Tuple] = {}

    @property
    def out_channels(self) -> int:
        return self.c2

    def emit(self, plan: Plan, x: View, out: Optional[View] = None, name: str = "transformerblock") -> View:
        if self.conv is not None:
            x = self.conv.emit(plan, x, name=name + ".conv")
        sig = _tensors_sig(self.linear.weight, self.linear.bias)
        hit = self._packed.get((plan.dtype, plan.device))
        if hit is None or hit[0] != sig:
            hit = self._packed[(plan.dtype, plan.device)] = (sig, fold_linear([(self.linear.weight,)], self.linear.bias, plan.dtype, plan.device))
        nl = len(self.tr)
        y = plan.conv(x, hit[1], 1, 0, ACT_NONE, out=out if nl == 0 else None, res=x, name=name + ".linear")
        for i, layer in enumerate(self.tr):
            y = layer.emit(plan, y, out=out if i == nl - 1 else None, name=f"{name}.tr.{i}")
        return y


class C3TR(C3):
    """C3 whose `m` is ONE TransformerBlock(c_, c_, 4, n) (reference common.py:362-367).  C3.emit's fused, strip and chained forms test isinstance(..., Bottleneck), so
    it takes the general path as C3Ghost does: cv1 + cv2 in one launch, the block through its own emit with its last launch writing into the concat half, cv3.
    Four heads of c_ / 4 channels: c2 * e must be 128, 256 or 512."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = TransformerBlock(c_, c_, 4, n)


class BottleneckCSP(HipModule):
    """cv4(LeakyReLU(BN(cat(cv3(m(cv1(x))), cv2(x))))) (reference :119-146; the r3.1 block: Hardswish in its Conv modules, LeakyReLU(0.1) after the shared BatchNorm).
    `cv2` and `cv3` are bare convolutions whose outputs meet in one BatchNorm over the concatenation: its first half is folded into cv3, its second into cv2, each
    followed by the LeakyReLU launch (Plan.conv with a legacy activation = convolution + ymi_act), both writing straight into the concat buffer cv4 reads."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1, version="r3.1")
        self.cv2 = nn.Conv2d(c1, c_, 1, 1, bias=False)
        self.cv3 = nn.Conv2d(c_, c_, 1, 1, bias=False)
        self.cv4 = Conv(2 * c_, c2, 1, 1, version="r3.1")
        self.bn = nn.BatchNorm2d(2 * c_, eps=BN_EPS, momentum=BN_MOMENTUM)
        self.act = nn.LeakyReLU(0.1, inplace=True)
        self.m = nn.Sequential(*[Bottleneck(c_, c_, shortcut, g, e=1.0, version="r3.1") for _ in range(n)])
        self._half: Dict[Tuple, Tuple] = {}

    @property
    def out_channels(self) -> int:
        return self.cv4.conv.out_channels

    def packed_half(self, which: int, dtype: torch.dtype, device: torch.device, cin_view: int) -> PackedConv:
        """cv3 (which = 0) / cv2 (which = 1) with its half of the shared BatchNorm folded in"""
        conv = self.cv3 if which == 0 else self.cv2
        c_ = conv.out_channels
        sl = slice(which * c_, (which + 1) * c_)
        bnp = (self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var)
        sig = tuple(t._version for t in (conv.weight,) + bnp) + (conv.weight.data_ptr(),)
        key = (which, dtype, device, cin_view)
        hit = self._half.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        pc = PackedConv(conv.weight, None, tuple(t[sl] for t in bnp) + (float(self.bn.eps),), dtype, device, cin_pad=cin_view)
        self._half[key] = (sig, pc)
        return pc

    def emit(self, plan: Plan, x: View, out: Optional[View] = None, name: str = "csp") -> View:
        c_ = self.cv1.conv.out_channels
        if c_ % 8:
            raise YmiError("BottleneckCSP hidden width must be a multiple of 8")
        cat = plan.alloc(x.n, x.h, x.w, 2 * c_)
        y = self.cv1.emit(plan, x, name=name + ".cv1")
        for j, b in enumerate(self.m):
            y = b.emit(plan, y, name=f"{name}.m.{j}")
        act = act_code(self.act)
        plan.conv(y, self.packed_half(0, plan.dtype, plan.device, y.c), 1, 0, act, out=cat.slice_c(0, c_), name=name + ".cv3+bn")
        plan.conv(x, self.packed_half(1, plan.dtype, plan.device, x.c), 1, 0, act, out=cat.slice_c(c_, c_), name=name + ".cv2+bn")
        return self.cv4.emit(plan, cat, out=out, name=name + ".cv4")


def focus_transform(x):
    """x(b,c,h,w) -> y(b,4c,h/2,w/2) (reference :237-240; the torch expression, for callers of the reference's helper -- the HIP path never materialises it)"""
    return torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)


def space_to_depth(x):
    """reference :243-249: the same rearrangement through view / permute"""
    n, c, h, w = x.size()
    x = x.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 5, 3, 1, 2, 4)
    return x.reshape(n, 4 * c, h // 2, w // 2)


class Focus(HipModule):
    """Conv(4 c1, c2, k) over the space-to-depth rearrangement of the image (reference :210-234), the stem of the r3.1 / r4.0 models.
    The rearrangement is never materialised: slot (dy, dx) of `focus_transform` holds pixel (2Y + dy, 2X + dx), so a k x k convolution with 'same' padding over the 12
    half-resolution channels IS a 2k x 2k stride-2 convolution over the image -- for the reference's k = 3: Conv(3, c2, 6, 2, 2) with
    W6[o, c, 2 ky + dy, 2 kx + dx] = W3[o, 3 slot(dy, dx) + c, ky, kx], slot = (0,0) (1,0) (0,1) (1,1) -> 0 1 2 3 (ultralytics/yolov5#4825, the equivalence the r6.0 stem was
    introduced with).  Same products, same zero padding, another summation order: the stem kernels (super-pixel form, planar-image form, fused stem + body.1) run unchanged."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True, version="r4.0"):
        super().__init__()
        self.conv = Conv(c1 * 4, c2, k, s, p, g, act, version=version)
        self._packed: Dict[Tuple, Tuple] = {}

    def _input_cpad(self, c: int) -> int:
        return 4

    def stem_weight(self) -> torch.Tensor:
        w = self.conv.conv.weight   # (c2, 4 c1, 3, 3)
        c2, c4, kh, kw = w.shape
        c1 = c4 // 4
        if (kh, kw) != (3, 3) or self.conv.conv.stride != (1, 1) or self.conv.conv.padding != (1, 1) or c1 != 3:
            raise NotImplementedError("Focus is emitted for the reference's stem only: 3 image channels, k = 3, s = 1, 'same' padding")
        w6 = w.new_zeros(c2, c1, 6, 6)
        for slot, (dy, dx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            w6[:, :, dy::2, dx::2] = w[:, slot * c1:(slot + 1) * c1]
        return w6

    def packed(self, dtype: torch.dtype, device: torch.device) -> PackedConv:
        cv = self.conv
        sig = tuple(t._version for t in (cv.conv.weight, cv.bn.weight, cv.bn.bias, cv.bn.running_mean, cv.bn.running_var)) + (cv.conv.weight.data_ptr(),)
        key = (dtype, device)
        hit = self._packed.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        bn = (cv.bn.weight, cv.bn.bias, cv.bn.running_mean, cv.bn.running_var, float(cv.bn.eps))
        pc = PackedConv(self.stem_weight(), None, bn, dtype, device, cin_pad=None, stem_superpixel=True)
        self._packed[key] = (sig, pc)
        return pc

    def emit(self, plan: Plan, x: View, out: Optional[View] = None, name: str = "focus") -> View:
        if x.c != 4:
            raise YmiError("Focus reads the NHWC4 image view (it is the network's first layer)")
        return plan.conv(x, self.packed(plan.dtype, plan.device), (2, 2), (2, 2), act_code(self.conv.act), out=out, name=name)


class SPP(HipModule):
    """cv2(cat(x, mp5(x), mp9(x), mp13(x))) after cv1 (reference :176-187)."""

    def __init__(self, c1, c2, k=(5, 9, 13), version="r4.0"):
        super().__init__()
        if tuple(k) != (5, 9, 13):
            raise NotImplementedError("the fused pool pyramid implements k=(5, 9, 13)")
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1, version=version)
        self.cv2 = Conv(c_ * (len(k) + 1), c2, 1, 1, version=version)
        self.m = nn.ModuleList([nn.MaxPool2d(kernel_size=x, stride=1, padding=x // 2) for x in k])

    def emit(self, plan: Plan, x: View, out: Optional[View] = None, name: str = "spp") -> View:
        c_ = self.cv1.conv.out_channels
        if c_ % 8:
            raise YmiError("SPP hidden width must be a multiple of 8")
        cat = plan.alloc(x.n, x.h, x.w, 4 * c_)
        self.cv1.emit(plan, x, out=cat.slice_c(0, c_), name=name + ".cv1")
        plan.spp_pool(cat, c_, name=name + ".pool")
        return self.cv2.emit(plan, cat, out=out, name=name + ".cv2")


class SPPF(SPP):
    """SPPF(k=5) == SPP(k=(5,9,13)) (reference :190-207, equivalence note :196); same parameters."""

    def __init__(self, c1, c2, k=5, version="r4.0"):
        if k != 5:
            raise NotImplementedError("the fused pool pyramid implements SPPF(k=5)")
        super().__init__(c1, c2, (5, 9, 13), version=version)
        self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)


class Classify(nn.Module):
    """Classification head, (b, c1, h, w) or a list of up to four such maps -> (b, c2) logits (reference :679-689: AdaptiveAvgPool2d(1) per map, torch.cat(..., 1), a
    1x1 Conv2d with bias, Flatten), as ONE launch of ops.classify_head: the maps are pooled straight into the GEMM's LDS block.  Same parameters as the reference's
    (`conv.weight`, `conv.bias`).  Limits: k = 1, s = 1, g = 1 (a pooled map is one pixel, so any other kernel is a different layer, and groups are not implemented);
    every map's channel count a multiple of 8; fp16 / bf16 compute (fp32-parameter modules compute in fp16 unless `compute_dtype` says bf16)."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1):
        super().__init__()
        if (k, s, g) != (1, 1, 1):
            raise NotImplementedError(f"Classify implements k = 1, s = 1, g = 1 only (got k = {k}, s = {s}, g = {g}): the pooled map is one pixel and grouped heads are out of scope")
        self.aap = nn.AdaptiveAvgPool2d(1)
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g)
        self.flat = nn.Flatten()

    def forward(self, x):
        from ... import ops
        from ...hipmodule import compute_dtype_of, nchw_to_view, weights_signature
        if self.training:
            raise NotImplementedError("yolort_amd implements the inference path only; call .eval() (training is out of scope)")
        xs = list(x) if isinstance(x, (list, tuple)) else [x]
        if not 1 <= len(xs) <= 4:
            raise YmiError(f"Classify takes one map or a list of up to four, got {len(xs)}")
        for t in xs:
            if not t.is_cuda:
                raise YmiError("yolort_amd runs on an MI355X only: move the model and inputs to 'cuda' (there is no CPU fallback)")
            if t.dim() != 4 or t.shape[1] % 8:
                raise YmiError(f"Classify expects NCHW maps whose channel count is a multiple of 8, got shape {tuple(t.shape)}")
        cdt = compute_dtype_of(self)
        if cdt == torch.float32:
            raise YmiError("the classifier head computes in float16 or bfloat16: compute_dtype = torch.float32 (the parity mode) has no head")
        with torch.cuda.device(xs[0].device):
            key = (cdt, xs[0].device.index, weights_signature(self))
            cached = self.__dict__.get("_ymi_head")
            if cached is None or cached[0] != key:
                cached = self.__dict__["_ymi_head"] = (key, ops.pack_linear(self.conv.weight, self.conv.bias, cdt))
            views = [nchw_to_view(None, t, t.shape[1], dtype=cdt) for t in xs]
            logits = ops.classify_head(views, cached[1], dtype=cdt)
        return logits.to(xs[0].dtype if xs[0].dtype.is_floating_point else torch.float32)
