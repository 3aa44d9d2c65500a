"""Mirror of the reference's `yolort.v5` import surface for the hot-path blocks only."""
from .models.common import C3, C3TR, SPP, SPPF, Bottleneck, BottleneckCSP, C3Ghost, Classify, Conv, DWConv, Focus, GhostBottleneck, GhostConv, QConv, TransformerBlock, TransformerLayer, autopad, focus_transform, space_to_depth  # noqa: F401
