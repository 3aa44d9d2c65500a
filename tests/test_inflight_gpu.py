"""Bit-stability of every launch's output while several batches are in flight.

The per-launch tests (tests/test_ops_gpu.py, tests/test_parity_gpu.py) run one launch alone on an idle device, and the lane simulator cannot see what only concurrency
shows: the asynchrony of LDS-DMA, a missing s_waitcnt, races between waves (tests/hipsim/README.md).  The product's headline mode keeps `pipeline_depth` plan instances in
flight on separate streams, and until now that mode was checked at the level of detections only, on yolov5n at 160 x 160 -- a plan that holds none of the pinned yolov5s
tiles, and a corrupted activation need not move a detection.

Here: the pinned headline plan (yolov5s fp16, batch 32, 640 x 640 -- the tiles are pinned per shape in yolort_amd/data/tiles_gfx950.json, a smaller batch would run other
kernels) and a small plan that takes the im2col-table path (yolov5m bf16, batch 2, 320 x 320).
  baseline     one synchronous forward on an idle device; every output a launch keeps (plan.io[idx]: y, y2, up2, chain_y, the strip kernel's y1_out) is cloned.  Buffers are not
               reused inside a plan, so they all survive the run; the per-launch parity test holds these very values to the oracle.
  in flight    the same batch submitted `pipeline_depth` (4) times with forward_async before any is collected; every kept output of every plan instance of the ring must
               equal the baseline BIT FOR BIT, and so must the detections.  10 rounds; 10 more with a second stream copying 64 MiB blocks throughout; one round through the
               other submit path (use_graph off: per-kernel enqueues).
This bounds the runtime: it is a check for stability, not an attempt to provoke anything.

Time limit: the test arms faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True).  A hang therefore ends the WHOLE pytest process with a traceback (and the reports of
the session's other tests with it) instead of sitting on the device: a stop-on-hang measure, chosen over a wait that nothing can interrupt from inside a blocked HIP call."""
import faulthandler

import pytest
import torch

pytestmark = pytest.mark.gpu

KEPT = ("y", "y2", "up2", "chain_y", "y1_out")
ROUNDS = 10
TIME_LIMIT_S = 240     # the whole test; a hang ends the process with a traceback instead of sitting on the device


@pytest.fixture(scope="module")
def dev():
    from yolort_amd import _lib
    _lib.load(require_gpu=True)
    return torch.device("cuda:0")


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _kept(plan):
    """(op index, key, view) of every output the plan's launches keep, in launch order"""
    out, seen = [], set()
    for idx in sorted(plan.io):
        for key in KEPT:
            v = plan.io[idx].get(key)
            if v is not None and (v.ptr, v.c, v.cs) not in seen:
                seen.add((v.ptr, v.c, v.cs))
                out.append((idx, key, v))
    return out


def _same_dets(a, b):
    return len(a) == len(b) and all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("boxes", "scores", "labels"))


def _compare(model, base, det0, dets, what):
    """every written kept output of every plan instance against the baseline; names the first differing op, tile and instance"""
    torch.cuda.synchronize()
    ring = [e for r in model._ring.values() for e in r]
    assert len(ring) == model.pipeline_depth, f"{what}: {len(ring)} plan instances for {model.pipeline_depth} batches in flight"
    for inst, e in enumerate(ring):
        for idx, key, v in _kept(e.plan):
            want = base.get((idx, key))
            if want is None:
                continue
            got = v.as_tensor()
            if not torch.equal(_bits(got), _bits(want)):
                d = _bits(got) != _bits(want)
                first = [int(i) for i in d.nonzero()[0]]
                raise AssertionError(f"{what}: op {idx} '{e.plan.names[idx]}' output '{key}' (tile {e.plan.meta[idx].get('tile')}, {e.plan.meta[idx].get('shape')}) of plan instance {inst} "
                                     f"differs from the idle-device baseline in {int(d.sum())} of {d.numel()} elements, first at (n, y, x, c) = {first}: "
                                     f"{float(got[tuple(first)])!r} instead of {float(want[tuple(first)])!r}")
    for j, d in enumerate(dets):
        assert _same_dets(det0, d), f"{what}: the detections of submission {j} differ from the synchronous run's"


@pytest.mark.parametrize("arch,dtype,n,size", [
    ("yolov5_darknet_pan_s_r60", torch.float16, 32, 640),     # the pinned headline plan: c3_tile, conv_halo8, conv3x3_rs, igemm8 ...
    ("yolov5_darknet_pan_m_r60", torch.bfloat16, 2, 320),     # widths 48 / 96 / 192: the im2col-table implicit GEMM
], ids=["yolov5s-fp16-bs32-640", "yolov5m-bf16-bs2-320"])
def test_every_kept_output_is_bit_stable_with_batches_in_flight(dev, arch, dtype, n, size):
    from yolort_amd.models import YOLOv5
    from workloads.synth import synth_images, synth_weights
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    try:
        m = YOLOv5(arch=arch, size=(size, size), score_thresh=0.25)
        m.load_state_dict(synth_weights(m.state_dict(), arch, seed=0, head_gain=0.5))
        m = m.to(dev).to(dtype).eval()
        model = m.model
        assert model.pipeline_depth == 4 and model.use_graph
        imgs = [im.to(dev).to(dtype) for im in synth_images(n, size, size, seed=1)]
        for _ in range(2):                                   # builds the first plan instance and captures its graph (twice: a first batch that overflows the candidate
            m.forward(imgs)                                  # capacity is redone on a rebuilt, larger plan, and the superseded instance leaves the ring with the next batch)
        torch.cuda.synchronize()
        assert len(model._ring) == 1 and len(next(iter(model._ring.values()))) == 1
        e0 = next(iter(model._entries.values()))
        assert e0 is next(iter(model._ring.values()))[0]
        kept = _kept(e0.plan)
        for _, _, v in kept:                                 # poison: an output the submit path never stores (the stem's, when stem + body.1 run as one launch) is not compared
            v.as_tensor().fill_(float("nan"))
        det0 = m.forward(imgs)                               # ---- the baseline: one synchronous forward on an idle device
        torch.cuda.synchronize()
        assert len(model._ring) == 1 and next(iter(model._ring.values())) == [e0]
        base, unwritten = {}, []
        for idx, key, v in kept:
            t = v.as_tensor()
            if bool(torch.isnan(t).all()):
                unwritten.append((idx, key, e0.plan.names[idx]))
            else:
                base[(idx, key)] = t.clone()
        print(f"INFLIGHT {arch}: {len(base)} kept outputs of {len(e0.plan.io)} launches, {sum(t.numel() * t.element_size() for t in base.values()) / 2**20:.0f} MiB; never stored: {unwritten}")
        assert len(base) >= len(e0.plan.io) - 1 and len(unwritten) <= 1, unwritten
        tiles = {e0.plan.meta[i].get("tile") for i in e0.plan.io}
        if n == 32:
            assert -3 in tiles and any(t is not None and t >= 91 for t in tiles), tiles   # the strip kernel and the pinned tiles are what runs

        def flight(what, noise=None):
            pend = []
            for _ in range(model.pipeline_depth):
                if noise is not None:
                    with torch.cuda.stream(noise[0]):
                        for _ in range(16):
                            noise[2].copy_(noise[1], non_blocking=True)   # memory traffic from another queue while the batches are in flight
                pend.append(m.forward_async(imgs))
            _compare(model, base, det0, [p.result() for p in pend], what)

        flight("the round that builds the other plan instances")   # (plans are built lazily between its submissions: compared like the rest, not counted)
        for r in range(ROUNDS):                              # from here on all four instances exist: four batches queued back to back
            flight(f"round {r}, {model.pipeline_depth} batches in flight")
        noise = (torch.cuda.Stream(device=dev), torch.empty(64 << 20, device=dev, dtype=torch.uint8), torch.empty(64 << 20, device=dev, dtype=torch.uint8))
        for r in range(ROUNDS):
            flight(f"round {r} with a second stream copying 64 MiB blocks", noise)
        torch.cuda.synchronize()
        model.use_graph = False                              # ---- the other submit path: per-kernel enqueues
        try:
            flight("per-kernel enqueues (use_graph off)")
        finally:
            model.use_graph = True
    finally:
        faulthandler.cancel_dump_traceback_later()
