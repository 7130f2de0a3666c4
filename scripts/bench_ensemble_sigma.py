#!/usr/bin/env python3
"""Cost of the sigma-weighted ensemble fusion beside the unweighted one, on the same points and probs in
one process.

    python scripts/bench_ensemble_sigma.py --out profiles/ensemble_sigma_bench.json

Four things are timed with HIP events, alternating window by window: SigmaEnsemblePoseSolver.fuse_batch and
Multi_Mean_PoseSolver.fuse_batch as a caller sees them (torch.stack of the M models' tensors, the output
allocations and the kernel), and the two C entries alone on preallocated buffers (back-to-back launches on
one stream: the launch rate bounds a kernel this short).  The median, minimum and maximum of the windows'
per-call means are reported.  No counters, no traces.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--models", type=int, default=4)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--queries", type=int, default=30)
    ap.add_argument("--classes", type=int, default=12)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--launches", type=int, default=2000)
    args = ap.parse_args()
    sys.path[:0] = [os.path.join(REPO, "satellite-pose-estimation_amd"), os.path.join(REPO, "tests")]
    import numpy as np
    import torch
    import ensemble_sigma_ref as es
    from spe import _lib
    from spe.solver import Multi_Mean_PoseSolver, SigmaEnsemblePoseSolver

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda:0")
    M, B, Q, C = args.models, args.batch, args.queries, args.classes
    pts, probs, sig, scale = es.ensemble_inputs(M, B, Q, C, seed=1, scaled=True)
    clip = np.concatenate([np.zeros((B, 2), np.float32), scale], 1)
    d = [[torch.from_numpy(np.ascontiguousarray(a[m])).to(dev) for m in range(M)] for a in (pts, probs, sig)]
    dclip = torch.from_numpy(clip).to(dev)
    sigma, mean = SigmaEnsemblePoseSolver(), Multi_Mean_PoseSolver()

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def stats(v):
        v = sorted(v)
        return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "windows": len(v)}

    # the C entries on preallocated buffers
    sp, sr, ss = (torch.stack(x).contiguous() for x in d)
    dscale = torch.from_numpy(scale).to(dev)
    f = sigma.fuse_batch(*d, clip_bbox=dclip)
    mp, mr = mean.fuse_batch(d[0], d[1])
    torch.cuda.synchronize()
    L = _lib.lib()
    a_sigma = [_lib.stream_ptr(), _lib.ptr(sp), _lib.ptr(sr), _lib.ptr(ss), _lib.ptr(dscale), M, B, Q, C, 1e-3, 3.0,
               _lib.ptr(f["points"]), _lib.ptr(f["probs"]), _lib.ptr(f["sigmas"]), _lib.ptr(f["n_pooled"]),
               _lib.ptr(f["n_kept"])]
    a_mean = [_lib.stream_ptr(), _lib.ptr(sp), _lib.ptr(sr), M, B, Q, C, _lib.ptr(mp), _lib.ptr(mr)]
    timed = {"fuse_batch_sigma": (lambda: sigma.fuse_batch(*d, clip_bbox=dclip), args.calls),
             "fuse_batch_mean": (lambda: mean.fuse_batch(d[0], d[1]), args.calls),
             "kernel_sigma": (lambda: L.spe_ensemble_fuse_sigma(*a_sigma), args.launches),
             "kernel_mean": (lambda: L.spe_ensemble_fuse(*a_mean), args.launches)}
    for fn, n in timed.values():
        window(fn, max(10, n // 10))
    times = {k: [] for k in timed}
    for _ in range(args.windows):
        for k, (fn, n) in timed.items():                    # the four alternate
            times[k].append(window(fn, n))
    res = {"what": "sigma-weighted (spe_ensemble_fuse_sigma) and unweighted (spe_ensemble_fuse) ensemble fusion on the "
                   "same points and probs, HIP events, per-window means of one call",
           "shape": {"models": M, "batch": B, "queries": Q, "classes": C}, "calls_per_window": args.calls,
           "launches_per_window": args.launches, "counters_or_traces": "none taken",
           "rows_emitted": int((f["n_kept"] > 0).sum().item()), "rows_gated_or_thinned": int((f["n_kept"] < f["n_pooled"]).sum().item()),
           "times": {k: stats(v) for k, v in times.items()}}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            json.dump(res, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
