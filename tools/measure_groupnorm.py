"""What the GroupNorm backbone (`--bn group_bn`, SpeConfig.norm) costs against the frozen-BN model of the same build,
on an MI355X: DETR at 416^2, 6 + 6 layers, B = 64 by default, bf16 and fp32.

  python tools/measure_groupnorm.py --time [--batch 64] [--rounds 3] [--iters 30] [--dtypes bf16,fp32]

A fresh process per sample (`--child`), the (norm, dtype) combinations interleaved over `--rounds` rounds, each sample
the median of `--iters` event-timed calls after a warm-up, of the backbone stage alone and of the whole forward.  A
group_bn child also reads the per-launch profiler for the two GroupNorm kinds: mean ms per forward and the bytes the
launch table charges them (stats: x once + the partials; apply: x, the residual where there is one, one write, the
partials), hence the achieved GB/s.  Prints one JSON document: the samples, the medians, the run-to-run spread of
each combination ((max - min) / median over its samples), group_bn over frozen_bn per dtype, and the GroupNorm
kinds' rates against a same-box copy figure (`--copy_tbs`, 5.4 TB/s: DESIGN.md).  Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "satellite-pose-estimation_amd"))

GN_KINDS = ("norm.gn.stats", "norm.gn.apply")


def gn_profile(m, fn, calls=5):
    """{kind: {ms, bytes, launches}} per forward, from the per-launch profiler over `calls` calls of fn"""
    import torch
    from spe import _lib
    L = _lib.lib()
    _lib.check(L.spe_model_profile_begin(m._h, b"norm.gn"), "spe_model_profile_begin")
    try:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    finally:
        n = L.spe_model_profile_end(m._h)
    out = {k: {"ms": 0.0, "bytes": 0.0, "launches": 0} for k in GN_KINDS}
    kb = ctypes.create_string_buffer(64)
    ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    for i in range(n):
        _lib.check(L.spe_model_profile_get(m._h, i, kb, 64, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)),
                   "spe_model_profile_get")
        r = out[kb.value.decode()]
        r["ms"] += ms.value / calls
        r["bytes"] += by.value / calls
        r["launches"] += 1
    for r in out.values():
        r["launches"] //= calls
        r["gb_per_s"] = r["bytes"] / (r["ms"] * 1e-3) / 1e9 if r["ms"] > 0 else None
    return out


def time_child(norm, dtype, B, iters):
    """One sample in this process: median ms of the backbone stage and of the whole forward."""
    import torch
    from spe.config import SpeConfig
    from spe.models import DETR
    from spe.synthetic import random_weights
    if not torch.cuda.is_available():
        raise SystemExit("measure_groupnorm: no GPU")
    cfg = SpeConfig(norm=norm)
    m = DETR(cfg, dtype=dtype)
    m.load_state_dict(random_weights(cfg, 0))
    dev = torch.device("cuda:0")
    x = torch.randn(B, 3, cfg.input_size, cfg.input_size, device=dev)
    ws = m.new_workspace(B, dev)

    def med(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    rec = {"norm": norm, "dtype": dtype, "backbone_ms": med(lambda: m.encode(x, ws, part="backbone")),
           "step_ms": med(lambda: m(x))}
    if norm == "group_bn":
        rec["kinds"] = gn_profile(m, lambda: m.encode(x, ws, part="backbone"))
    print(json.dumps(rec))


def time_all(B, rounds, iters, dtypes, copy_tbs):
    combos = [(n, d) for d in dtypes for n in ("frozen_bn", "group_bn")]
    samples = {f"{n}-{d}": [] for n, d in combos}
    for _ in range(rounds):
        for n, d in combos:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--norm", n, "--dtype", d,
                                "--batch", str(B), "--iters", str(iters)], capture_output=True, text=True, timeout=400)
            if r.returncode != 0:
                raise SystemExit(f"child failed ({n}, {d}): {r.stderr[-2000:]}")
            samples[f"{n}-{d}"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"batch": B, "input_size": 416, "iters": iters, "rounds": rounds, "copy_tb_per_s": copy_tbs, "samples": samples}
    for name, ss in samples.items():
        for key in ("backbone_ms", "step_ms"):
            v = [s[key] for s in ss]
            out[f"{name}_{key}_median"] = statistics.median(v)
            out[f"{name}_{key}_spread"] = (max(v) - min(v)) / statistics.median(v)
    for d in dtypes:
        for key in ("backbone_ms", "step_ms"):
            out[f"group_over_frozen_{d}_{key}"] = out[f"group_bn-{d}_{key}_median"] / out[f"frozen_bn-{d}_{key}_median"]
        kinds = {}
        for k in GN_KINDS:
            ms = [s["kinds"][k]["ms"] for s in samples[f"group_bn-{d}"]]
            by = samples[f"group_bn-{d}"][0]["kinds"][k]["bytes"]
            med = statistics.median(ms)
            kinds[k] = {"ms_per_forward_median": med, "ms_spread": (max(ms) - min(ms)) / med, "bytes_per_forward": by,
                        "launches": samples[f"group_bn-{d}"][0]["kinds"][k]["launches"],
                        "gb_per_s": by / (med * 1e-3) / 1e9, "fraction_of_copy": by / (med * 1e-3) / (copy_tbs * 1e12)}
        out[f"kinds_{d}"] = kinds
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--norm", default="group_bn")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--copy_tbs", type=float, default=5.4)
    a = ap.parse_args()
    if a.child:
        time_child(a.norm, a.dtype, a.batch, a.iters)
    elif a.time:
        time_all(a.batch, a.rounds, a.iters, a.dtypes.split(","), a.copy_tbs)
    else:
        ap.error("--time (on a GPU)")
