"""Input-transform launch times on SPEED-sized synthetic frames: the validation transform
(spe_preprocess) and the submission transform (spe_preprocess_submission) on the same frames and
boxes, in one process, HIP events after warm-up.

usage: python scripts/preprocess_bench.py [--batch 64] [--size 416] [--inner 50] [--rounds 10] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "satellite-pose-estimation_amd"))
from spe import _lib  # noqa: E402
from spe.datasets import SpeedSubmissionTransform, SpeedValTransform  # noqa: E402
from spe.synthetic import synthetic_frames  # noqa: E402


def timed(fns, inner, rounds, warmup):
    """Per-launch milliseconds of each fn: `rounds` event-bracketed windows of `inner` back-to-back
    launches, the fns alternating window by window."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for k, v in ev.items():
        ms = np.array([a.elapsed_time(b) for a, b in v]) / inner
        out[k] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    d = synthetic_frames(8, seed=3)
    idx = np.arange(a.batch) % 8
    dev = torch.device("cuda", 0)
    frames = torch.from_numpy(d["frames"][idx]).to(dev)
    bbox = torch.from_numpy(d["bbox_xxyy"][idx]).to(dev)
    B, H, W = frames.shape
    S = a.size
    ov = SpeedValTransform(S)(frames, bbox)
    ob = SpeedSubmissionTransform(S)(frames, bbox, crops=True)
    torch.cuda.synchronize()
    assert (ov["status"] == 0).all() and (ob["status"] == 0).all()
    # the C entry points directly, so a window holds launches and nothing else
    L, st, P = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    fr, bb = P(frames), P(bbox)
    args = (st, fr, B, H, W, 1, bb, S)
    fns = {"spe_preprocess": lambda: L.spe_preprocess(*args, P(ov["images"]), P(ov["clip_bbox"]), P(ov["status"])),
           "spe_preprocess_submission": lambda: L.spe_preprocess_submission(
               *args, P(ob["images"]), None, P(ob["clip_bbox"]), P(ob["status"])),
           "spe_preprocess_submission_u8_only": lambda: L.spe_preprocess_submission(
               *args, None, P(ob["crops"]), P(ob["clip_bbox"]), P(ob["status"]))}
    res = {"batch": B, "frame": [H, W], "size": S, "inner": a.inner, "rounds": a.rounds}
    res.update(timed(fns, a.inner, a.rounds, a.warmup))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
