"""Generates tests/golden/crop_rects.json: boxes, parameters and the integer rectangles the REFERENCE cuts for them -- save_one_box's arithmetic
(yolort/v5/utils/plots.py:545-558) through the reference's own xyxy2xywh, xywh2xyxy and clip_coords (yolort/v5/utils/general.py), called in save_one_box's order.
save_one_box itself is not called: it needs cv2.  (oracle.reference_loader.load_reference() imports the whole reference package, yolort.v5.utils.plots included,
whose import looks for a font and tries to fetch it where it is missing.)  Build container only (needs the reference):

    python tests/golden/make_crop_golden.py

The rectangles are stored as the reference leaves them (an empty one keeps its clipped corners); the boxes as the doubles that equal their fp32 values."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

F32 = np.float32
GROUPS = (   # (h, w, gain, pad, square)
    (48, 64, 1.02, 10, False),     # save_one_box's defaults
    (37, 53, 1.3, 30, True),       # apply_classifier's recipe
    (48, 64, 1.0, 0, False),       # the bare box
    (8, 8, 1.02, 10, True),
    (37, 53, 1.0, 0, True),
)


def reference_rects(G, boxes, h, w, gain, pad, square):
    xyxy = torch.tensor(boxes, dtype=torch.float32).view(-1, 4)
    b = G.xyxy2xywh(xyxy)                                    # plots.py:548
    if square:
        b[:, 2:] = b[:, 2:].max(1)[0].unsqueeze(1)           # plots.py:550
    b[:, 2:] = b[:, 2:] * gain + pad                         # plots.py:551
    r = G.xywh2xyxy(b).long()                                # plots.py:552
    G.clip_coords(r, (h, w))                                 # plots.py:553
    return r, G.xywh2xyxy(b)


def near_integer_boxes(G, h, w, gain, pad, square, rng, want=8):
    """boxes whose left (or top) corner after `* gain + pad` lies within an ulp of an integer: x1 is walked ulp by ulp around the solution of corner = t"""
    out = []
    for _ in range(400):
        if len(out) >= want:
            break
        horizontal = bool(rng.integers(2))
        lim = w if horizontal else h
        t = int(rng.integers(1, max(lim - 2, 2)))
        side = float(rng.uniform(2.0, lim / 2))
        box = [0.0, 0.0, 0.0, 0.0]
        o = 0 if horizontal else 1
        box[1 - o], box[3 - o] = 1.0, 1.0 + (side if square else float(rng.uniform(1.0, 6.0)))   # under `square` both sides are equal: this one is the larger
        # corner = cx - (side * gain + pad) / 2 = t  ->  x1 = t + (side * (gain - 1) + pad) / 2
        x1 = F32(t + (side * (gain - 1.0) + pad) / 2.0)
        for _ in range(64):
            x1 = np.nextafter(x1, F32(-np.inf))
        for _ in range(128):
            x1 = np.nextafter(x1, F32(np.inf))
            box[o], box[o + 2] = float(x1), float(F32(x1 + F32(side)))
            _, corners = reference_rects(G, [box], h, w, gain, pad, square)
            c = F32(corners[0, o].item())
            if c in (F32(t), np.nextafter(F32(t), F32(-np.inf)), np.nextafter(F32(t), F32(np.inf))):
                out.append(list(box))
                if len(out) % 3 == 0:
                    break
    return out[:want]


def group_boxes(G, h, w, gain, pad, square, rng):
    u = lambda lo, hi: float(F32(rng.uniform(min(lo, hi), max(lo, hi))))   # (the 8 x 8 image turns some of the ranges below around)
    boxes = []
    for _ in range(12):                                                       # inside
        x1, y1 = u(0, w * 0.7), u(0, h * 0.7)
        boxes.append([x1, y1, float(F32(x1 + u(1, w * 0.3))), float(F32(y1 + u(1, h * 0.3)))])
    boxes += [[u(-9, -1), u(2, h / 2), u(3, w / 2), u(h / 2, h - 1)], [u(w / 2, w - 2), u(2, h / 2), u(w + 1, w + 9), u(h / 2, h - 1)],       # straddle left / right
              [u(2, w / 2), u(-9, -1), u(w / 2, w - 1), u(3, h / 2)], [u(2, w / 2), u(h / 2, h - 2), u(w / 2, w - 1), u(h + 1, h + 9)],       # top / bottom
              [u(-9, -1), u(-9, -1), u(3, w / 2), u(3, h / 2)], [u(w / 2, w - 2), u(h / 2, h - 2), u(w + 1, w + 9), u(h + 1, h + 9)],         # two corners
              [u(-9, -1), u(-9, -1), u(w + 1, w + 9), u(h + 1, h + 9)]]                                                                         # all four edges
    boxes += [[u(-90, -60), u(2, h - 2), u(-59, -50), u(2, h - 2) + 3], [u(w + 50, w + 60), 2.0, u(w + 61, w + 90), 9.0],                       # wholly outside
              [3.0, u(-90, -60), 9.0, u(-59, -50)], [3.0, u(h + 50, h + 60), 9.0, u(h + 61, h + 90)]]
    for _ in range(4):                                                        # thinner than a pixel (one side or both)
        x1, y1 = u(1, w - 2), u(1, h - 2)
        boxes.append([x1, y1, float(F32(x1 + u(0.01, 0.9))), float(F32(y1 + (u(0.01, 0.9) if rng.integers(2) else u(2, 5))))])
    boxes += near_integer_boxes(G, h, w, gain, pad, square, rng)
    boxes += [[u(5, w / 2), u(1, 4), u(5, w / 2) + 2.5, u(h - 6, h - 1)], [u(1, 4), u(5, h / 2), u(w - 6, w - 1), u(5, h / 2) + 2.5],           # tall, wide (what `square` changes)
              [10.25, 3.5, 12.75, float(h) - 2.25], [2.5, 9.75, float(w) - 3.5, 11.25]]
    boxes += [[u(w / 2, w - 1), 4.0, u(1, w / 2 - 1), 20.0], [4.0, u(h / 2, h - 1), 20.0, u(1, h / 2 - 1)]]                                       # inverted
    boxes += [[0.0, 0.0, float(w), float(h)], [5.0, 5.0, 5.0, 5.0]]                                                                               # the whole image, a point
    return [[float(F32(v)) for v in b] for b in boxes]


def main():
    from oracle.reference_loader import load_reference
    load_reference()
    from yolort.v5.utils import general as G
    rng = np.random.default_rng(20240)
    groups, total = [], 0
    for h, w, gain, pad, square in GROUPS:
        boxes = group_boxes(G, h, w, gain, pad, square, rng)
        rects, _ = reference_rects(G, boxes, h, w, gain, pad, square)
        groups.append(dict(h=h, w=w, gain=gain, pad=pad, square=square, boxes=boxes, rects=rects.tolist()))
        total += len(boxes)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "crop_rects.json")
    with open(out, "w") as f:
        json.dump(dict(source="yolort/v5/utils/general.py xyxy2xywh, xywh2xyxy, clip_coords in the order of yolort/v5/utils/plots.py:548-553", groups=groups), f, indent=0)
    print(f"{out}: {total} boxes in {len(groups)} groups")


if __name__ == "__main__":
    main()
