"""Times the exhaustive four-point-subset solver (spe_pnp_exhaustive) on the device.

HIP events around `reps` back-to-back solves on one stream, after a warm-up; the median of `windows`
such windows, per call.  Shapes: B = 64, Q = 11 and Q = 30, topk 1 / 10 / 32.  Per shape: the whole
solve, its two stages separately (spe_debug_pnp_exhaustive_stages: 1 = hypotheses, 2 = selection +
refinement on the records stage 1 left), and modes 2 (EPnP-RANSAC + sigma LM) and 4 (EPnP + Ceres LM) on
the same inputs in the same process.  On tests/helpers.solver_stress_set it also records each mode's
mean SPEED score (s_t + s_q over all images, failures as zero poses) against the set's ground truth.

    python tools/measure_pnp_exhaustive.py [--out profiles/pnp_exhaustive_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "satellite-pose-estimation_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import solver_stress_set  # noqa: E402
from spe import _lib  # noqa: E402
from spe.solver import EPnPCeresSolver, ExhaustivePoseSolver, SimplePoseSolverSigma  # noqa: E402
from spe.speed_eval import speed_score  # noqa: E402


def timed(fn, warmup, reps, windows):
    """median over `windows` of (event time of `reps` calls) / reps, in ms; also min and max."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def stage_call(solver, pts, probs, sig, out, stages):
    B, Q, C = probs.shape
    Kd, Wd = solver._consts(probs.device)

    def fn():
        _lib.check(_lib.lib().spe_debug_pnp_exhaustive_stages(
            _lib.stream_ptr(None), _lib.ptr(pts), _lib.ptr(probs), _lib.ptr(sig), B, Q, C, _lib.ptr(Kd), _lib.ptr(Wd),
            solver.reprojectionError, solver.topk, _lib.ptr(out["quat"]), _lib.ptr(out["tvec"]), _lib.ptr(out["rvec"]),
            _lib.ptr(out["status"]), _lib.ptr(out["n_corr"]), _lib.ptr(out["corr_label"]),
            _lib.ptr(out["inlier_mask"]), None, _lib.ptr(out["cand_index"]), _lib.ptr(out["repro_final"]), stages),
            "spe_debug_pnp_exhaustive_stages")
    return fn


def mean_score(o, q_gt, t_gt):
    q, t = o["quat"].double().cpu().numpy(), o["tvec"].cpu().numpy()
    s = [sum(speed_score(q[i], t[i], q_gt[i], t_gt[i])) for i in range(len(q))]
    return float(np.mean(s)), float(np.median(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pnp_exhaustive_bench.json"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "warmup": a.warmup, "reps": a.reps,
           "windows": a.windows, "timing": "HIP events around `reps` calls on one stream, median of `windows`",
           "shapes": []}
    tw = dict(warmup=a.warmup, reps=a.reps, windows=a.windows)
    for Q in (11, 30):
        pts, probs, q_gt, t_gt, sig = solver_stress_set(a.batch, seed=0, Q=Q)
        P, R, S = (torch.from_numpy(x).to(dev) for x in (pts, probs, sig))
        row = {"Q": Q, "n_corr_mean": None, "modes": {}, "exhaustive": {}}
        m2, m4 = SimplePoseSolverSigma(), EPnPCeresSolver()
        th4 = torch.full((a.batch,), 20.0, device=dev)
        for name, fn in (("mode2_epnp_ransac_sigma", lambda: m2.solve_batch(P, R, S)),
                         ("mode4_epnp_ceres_th20", lambda: m4.solve_batch(P, R, S, repro_per_image=th4))):
            o = fn()
            torch.cuda.synchronize()
            mean, med = mean_score(o, q_gt, t_gt)
            row["modes"][name] = dict(timed(fn, **tw), speed_score_mean=mean, speed_score_median=med,
                                      solved=int((o["status"] == 0).sum()))
        for topk in (1, 10, 32):
            ex = ExhaustivePoseSolver(topk=topk)
            out = ex.solve_batch(P, R, S)
            torch.cuda.synchronize()
            mean, med = mean_score(out, q_gt, t_gt)
            row["n_corr_mean"] = float(out["n_corr"].float().mean())
            e = {"solve": timed(lambda: ex.solve_batch(P, R, S, out=out), **tw),
                 "stage1_hypotheses": timed(stage_call(ex, P, R, S, out, 1), **tw),
                 "stage2_select_refine": timed(stage_call(ex, P, R, S, out, 2), **tw),
                 "speed_score_mean": mean, "speed_score_median": med, "solved": int((out["status"] == 0).sum())}
            row["exhaustive"][f"topk{topk}"] = e
        res["shapes"].append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
