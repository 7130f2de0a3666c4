#!/usr/bin/env python3
"""Cost of the landmark reconstruction (spe.landmarks): solve() at N = 12 000 views, L = 11, 10 LM steps
(the size of SPEED's training set), update() on a batch of 64 model outputs, and the numpy restatement
(tests/landmarks_ref.py) on the same observations on the CPU, for scale.

    python scripts/bench_landmarks.py --out profiles/landmarks_bench.json

Times are HIP events around `launches` calls per window on the current stream; the median, the minimum and
the maximum of the windows are reported.  solve_device() is what is timed for the solve (the launch sequence
and its output allocation, no download); update() writes into the same rows every time (the row counter is
put back), so the buffers do not grow while it is measured.  No counters, no traces.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "satellite-pose-estimation_amd"), os.path.join(REPO, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=12000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "landmarks_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import landmarks_ref as lr
    from spe.config import Camera, world_points
    from spe.landmarks import LandmarkReconstruction

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda:0")
    W, K = world_points(), np.asarray(Camera.K, np.float64)
    N, B = args.views, args.batch
    d = lr.model_outputs(N, W, K, seed=0, Q=30)
    t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}

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

    rec = LandmarkReconstruction(11)
    for i in range(0, N, 1000):
        s = slice(i, min(i + 1000, N))
        rec.update(t["points"][s], t["probs"][s], t["sigmas"][s], t["q"][s], t["t"][s], sigma_scale=t["scale"][s])
    model = rec.solve(args.iterations)
    solve = lambda: rec.solve_device(args.iterations)
    window(solve, 3)
    t_solve = stats([window(solve, args.launches) for _ in range(args.windows)])

    s = slice(0, B)
    n0 = rec.n - B

    def update():
        rec.n = n0
        rec.update(t["points"][s], t["probs"][s], t["sigmas"][s], t["q"][s], t["t"][s], sigma_scale=t["scale"][s])

    window(update, 3)
    t_update = stats([window(update, args.launches) for _ in range(args.windows)])

    px, sg, valid = lr.select_observations(d["points"], d["probs"], d["sigmas"], d["scale"])
    c0 = time.perf_counter()
    ref = lr.solve(px, sg, valid, d["q"], d["t"], K, iterations=args.iterations)
    cpu_ms = (time.perf_counter() - c0) * 1e3
    out = {"device": torch.cuda.get_device_name(0), "views": N, "landmarks": 11, "iterations": args.iterations,
           "batch": B, "launches_per_window": args.launches,
           "solve_device": t_solve, "update": t_update, "numpy_restatement_cpu_ms": cpu_ms,
           "largest_distance_to_truth_m": float(model.compare(W).max()),
           "largest_difference_to_restatement_m": float(np.abs(model.points - ref["world"]).max()),
           "not_measured": "the kernels' device time alone, the download in solve(), other N / L, a lens"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
