"""Mirror of the reference's `yolort.v5` import surface for the hot-path blocks only."""
from .models.common import C3, SPP, SPPF, Bottleneck, BottleneckCSP, C3Ghost, Classify, Conv, DWConv, Focus, GhostBottleneck, GhostConv, autopad, focus_transform, space_to_depth  # noqa: F401
