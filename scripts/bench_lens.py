#!/usr/bin/env python3
"""Cost of the lens step (spe_undistort_points): the launch alone at B = 64, Q = 11 and Q = 30, with and
without sigmas, and the PosePipeline step (RT-DETR r18, bf16, sigma solver) without and with a lens,
beside another build of the project (the parent commit) in the same call.

    python scripts/bench_lens.py --parent-pkg DIR --out profiles/lens_bench.json

DIR is the parent commit's package directory (its satellite-pose-estimation_amd/, built).  One fresh
process per tree, in the order parent, this tree, parent, so the two parent runs give the run-to-run
spread of a step that has no lens code in it.  Inside a process the modes alternate window by window.
Times are HIP events around `steps` pipeline steps (or `launches` kernel launches) per window; the
median, the minimum and the maximum of the windows are reported.  No counters, no traces.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# calibration-like magnitudes (tests/lens_ref.py)
DIST = [-0.22383016606510672, 0.51409797089106379, -0.00066499611998340662, -0.00021404771667484594,
        -0.13124227429077406]


def child(args):
    sys.path[:0] = [args.pkg]
    os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
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
    has_lens = "spe_undistort_points" in _lib.EXPORTS
    cfg = RtdetrConfig(depth=18)
    model = RTDETR(cfg, dtype="bf16", aux_outputs=False)
    model.load_state_dict(random_rtdetr_weights(cfg, 0))
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

    pipes = {}
    for mode in (["off", "on"] if has_lens else ["off"]):
        ns = argparse.Namespace(solver="epnp_ransac_sigma", **({"dist": DIST} if mode == "on" else {}))
        p = PosePipeline(model, build_solver(ns), B, device=dev)
        p.load(images, clip)
        pipes[mode] = p
    for p in pipes.values():
        window(p.run, args.warmup)
    times = {m: [] for m in pipes}
    for _ in range(args.windows):
        for m, p in pipes.items():                          # the modes alternate
            times[m].append(window(p.run, args.steps))
    res = {"tree": args.tree, "batch": B, "model": "rtdetr_r18", "dtype": "bf16", "input_size": cfg.input_size,
           "num_queries": cfg.num_queries, "solver": "epnp_ransac_sigma", "steps_per_window": args.steps,
           "step": {m: stats(v) for m, v in times.items()}}
    if has_lens:
        res["pipeline_lens_status_nonzero"] = int(pipes["on"].out["poses"]["lens_status"].count_nonzero())
        # launches only: preallocated arrays through the C entry, no tensor allocation in the window
        L = _lib.lib()
        Kd = torch.tensor([[3003.4, 0, 960], [0, 3003.4, 600], [0, 0, 1]], dtype=torch.float64, device=dev)
        dd = torch.tensor(DIST, dtype=torch.float64, device=dev)
        res["kernel"] = {}
        for Q in (11, 30):
            pts = (torch.rand(B, Q, 2, generator=g) * torch.tensor([1920.0, 1200.0])).to(dev)
            sig = (torch.rand(B, Q, 2, generator=g) * 2 + 0.5).to(dev)
            out, sout = torch.empty_like(pts), torch.empty_like(sig)
            st = torch.empty(B, Q, dtype=torch.uint8, device=dev)
            for name, s, so in (("points", None, None), ("points_and_sigmas", sig, sout)):
                argv = [_lib.stream_ptr(), _lib.ptr(pts), _lib.ptr(s), None, B, Q, _lib.ptr(Kd), _lib.ptr(dd), 5,
                        _lib.ptr(out), _lib.ptr(so), _lib.ptr(st)]
                launch = lambda: L.spe_undistort_points(*argv)
                _lib.check(launch(), "spe_undistort_points")
                window(launch, args.launches)
                r = stats([window(launch, args.launches) for _ in range(args.windows)])
                r["launches_per_window"] = args.launches
                r["status_nonzero"] = int(st.count_nonzero())
                res["kernel"][f"B{B}_Q{Q}_{name}"] = r
        res["kernel_note"] = "back-to-back launches on one stream: launch rate bound for a kernel this short"
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
    doc = {"what": "PosePipeline step (rtdetr_r18, bf16, sigma solver) without / with a lens on the solver and "
                   "spe_undistort_points alone, HIP events, per-window means; parent = the commit before the lens",
           "counters_or_traces": "none taken", "runs": runs}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
