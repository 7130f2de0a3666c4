#!/usr/bin/env python3
"""Cost of the calibration records (spe_calibration_records): the call alone on 64 solved poses and the
PosePipeline step (pose_cov on) without and with a Calibration.update, beside another build of the
project (the parent commit) in the same call.

    python scripts/bench_calibration.py --parent-pkg DIR --out profiles/calibration_bench.json

DIR is the parent commit's package directory (its satellite-pose-estimation_amd/, built).  One fresh
process per tree, in the order parent, this tree, parent, so the two parent runs give the run-to-run
spread of a step that has no calibration code in it.  Inside a process the modes alternate window by
window.  Times are HIP events around `steps` pipeline steps (or `launches` kernel launches) per window;
the median, the minimum and the maximum of the windows are reported.  No counters, no traces.  The
accumulator is emptied between windows (its list of per-batch device tensors would otherwise grow with
the window count); summarize() is not timed.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    sys.path[:0] = [args.pkg, os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")]
    os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
    import numpy as np
    import torch
    from spe import _lib
    from spe.pipeline import PosePipeline
    from spe.rtdetr import RTDETR
    from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights
    from spe.solver import build_solver

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda:0")
    B = args.batch
    try:
        from spe.calibration import Calibration
    except ImportError:
        Calibration = None
    cfg = RtdetrConfig(depth=18)
    model = RTDETR(cfg, dtype="bf16", aux_outputs=False)
    model.load_state_dict(random_rtdetr_weights(cfg, 0))
    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma"))
    g = torch.Generator().manual_seed(0)
    images = torch.randn(B, 3, cfg.input_size, cfg.input_size, generator=g).to(dev)
    xy = torch.rand(B, 2, generator=g) * 600
    clip = torch.cat([xy, xy + 200 + torch.rand(B, 1, generator=g) * 500], 1).to(dev)

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

    pipes, cal = {}, None
    for mode in (["cov", "cov+calibration"] if Calibration is not None else ["cov"]):
        kw = {}
        if mode != "cov":
            cal = Calibration(solver=solver)
            kw = dict(calibration=cal)
        p = PosePipeline(model, solver, B, device=dev, pose_cov=True, **kw)
        p.load(images, clip)
        pipes[mode] = p
    for p in pipes.values():
        window(p.run, args.warmup)
    times = {m: [] for m in pipes}
    for _ in range(args.windows):
        for m, p in pipes.items():                          # the modes alternate
            if cal is not None:
                cal.batches.clear()
            times[m].append(window(p.run, args.steps))
    res = {"tree": args.tree, "batch": B, "model": "rtdetr_r18", "dtype": "bf16", "input_size": cfg.input_size,
           "solver": "epnp_ransac_sigma", "steps_per_window": args.steps,
           "step": {m: stats(v) for m, v in times.items()}}
    if Calibration is not None:
        o = pipes["cov+calibration"].out
        res["pipeline_calib_status_counts"] = torch.bincount(o["calibration"]["calib_status"], minlength=5).tolist()
        # the call alone on solved poses: synthetic keypoints (tests/helpers.py) through the sigma solver
        from helpers import solver_stress_set
        pts, probs, q, t, sig = solver_stress_set(B, seed=7, Q=11, C=12, degenerate_frac=0.0)
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pts, probs, sig)]
        q_gt = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float64)).to(dev)
        t_gt = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(dev)
        poses = solver.solve_batch(*d)
        cov = solver.pose_covariance(d[1], d[2], poses)
        from spe.calibration import RECORDS, calibration_records
        out = calibration_records(d[0], d[1], d[2], poses, cov, q_gt, t_gt, solver=solver)
        torch.cuda.synchronize()
        res["kernel_calib_status_counts"] = torch.bincount(out["calib_status"], minlength=5).tolist()
        # launches only: preallocated outputs through the C entry, no tensor allocation in the window
        Kd, Wd = solver._consts(dev)
        L = _lib.lib()
        argv = [_lib.stream_ptr(), _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), None, 1e-3, _lib.ptr(poses["status"]),
                _lib.ptr(poses["corr_label"]), _lib.ptr(poses["inlier_mask"]), _lib.ptr(poses["rvec"]),
                _lib.ptr(poses["tvec"]), _lib.ptr(q_gt), _lib.ptr(t_gt), _lib.ptr(cov["pose_cov"]),
                _lib.ptr(cov["cov_status"]), B, 11, 12, _lib.ptr(Kd), _lib.ptr(Wd), 1.0] + [_lib.ptr(out[k]) for k in RECORDS]
        launch = lambda: L.spe_calibration_records(*argv)
        window(launch, args.launches)
        res["kernel"] = stats([window(launch, args.launches) for _ in range(args.windows)])
        res["kernel"]["launches_per_window"] = args.launches
        res["kernel"]["note"] = "back-to-back launches on one stream: launch rate bound for a kernel this short"
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default="this")
    ap.add_argument("--pkg", default=os.path.join(REPO, "satellite-pose-estimation_amd"))
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--launches", type=int, default=2000)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    trees = [("this", args.pkg)] if args.parent_pkg is None else [("parent", args.parent_pkg), ("this", args.pkg),
                                                                   ("parent", args.parent_pkg)]
    for name, pkg in trees:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--pkg", pkg, "--tree", name] + [
            f"--{k}={getattr(args, k)}" for k in ("batch", "windows", "steps", "warmup", "launches")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            # a failed run ends the measurement: nothing more is started on the device
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"{name}: child failed with code {r.returncode}")
        rec = json.loads(line[0][7:])
        runs.append(rec)
        print(name, json.dumps(rec["step"]), json.dumps(rec.get("kernel", {})), flush=True)
    doc = {"what": "PosePipeline step (rtdetr_r18, bf16, sigma solver, pose_cov on) without / with Calibration.update and "
                   "spe_calibration_records alone, HIP events, per-window means; parent = the commit before the calibration",
           "counters_or_traces": "none taken", "runs": runs}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
