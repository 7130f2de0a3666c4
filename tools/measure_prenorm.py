"""A/B of the pre-norm DETR model (SpeConfig.pre_norm) against the post-norm model of the same build: both do the
same GEMM and attention work, so post-norm is the yardstick.

B = 64, 416^2, Q = 11, 6/6 layers, bf16.  HIP-event timed; every model is measured `--repeats` times (default 3),
alternating pre / post, each repeat the median of `--iters` calls: ms per forward and the backbone, transformer
(encoder) and decode stage times, with the run-to-run spread over the repeats.  The per-launch tables of both
models (spe_model_profile_*: kind, ms) are recorded too, summed per kind.

Usage: python tools/measure_prenorm.py [--out profiles/prenorm_ab.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "satellite-pose-estimation_amd"))


def launch_rows(m, call):
    """[[kind, ms], ...] of one call, in issue order"""
    import torch

    from spe import _lib
    L = _lib.lib()
    _lib.check(L.spe_model_profile_begin(m._h, b""), "spe_model_profile_begin")
    try:
        call()
        torch.cuda.synchronize()
    finally:
        n = L.spe_model_profile_end(m._h)
    kb = ctypes.create_string_buffer(64)
    ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    rows = []
    for i in range(n):
        _lib.check(L.spe_model_profile_get(m._h, i, kb, 64, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)),
                   "spe_model_profile_get")
        rows.append([kb.value.decode(), ms.value])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "prenorm_ab.json"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch

    from spe.config import SpeConfig
    from spe.models import DETR
    from spe.synthetic import random_weights, synthetic_batch
    dev = torch.device("cuda:0")
    B = args.batch
    models, imgs, wss = {}, {}, {}
    for name, pre in (("post_norm", False), ("pre_norm", True)):
        cfg = SpeConfig(pre_norm=pre)
        m = DETR(cfg, dtype="bf16")
        m.load_state_dict(random_weights(cfg, 0))
        one = torch.from_numpy(synthetic_batch(cfg, 4, 1)["images"]).to(dev)
        models[name], imgs[name] = m, one.repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous()
        wss[name] = m.new_workspace(B, dev)

    def time_ms(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    samples = {n: {"forward_ms": [], "backbone_ms": [], "encoder_ms": [], "decoder_ms": []} for n in models}
    for _ in range(args.repeats):
        for name, m in models.items():
            img, ws = imgs[name], wss[name]
            s = samples[name]
            s["forward_ms"].append(time_ms(lambda: m(img)))
            s["backbone_ms"].append(time_ms(lambda: m.encode(img, ws, part="backbone")))
            s["encoder_ms"].append(time_ms(lambda: m.encode(None, ws, part="transformer", B=B)))
            s["decoder_ms"].append(time_ms(lambda: m.decode(B, ws)))
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "input_size": 416, "queries": 11, "layers": "6/6",
           "dtype": "bf16", "warmup": args.warmup, "iters": args.iters, "repeats": args.repeats}
    for name, m in models.items():
        r = {}
        for k, v in samples[name].items():
            r[k] = statistics.median(v)
            r[k + "_samples"] = v
            r[k + "_spread"] = max(v) - min(v)
        rows = launch_rows(m, lambda: m(imgs[name]))
        per_kind = {}
        for kind, ms in rows:
            e = per_kind.setdefault(kind, {"launches": 0, "ms": 0.0})
            e["launches"] += 1
            e["ms"] += ms
        r["launches"] = len(rows)
        r["launch_kinds"] = [k for k, _ in rows]
        r["per_kind"] = per_kind
        res[name] = r
    for k in ("forward_ms", "backbone_ms", "encoder_ms", "decoder_ms"):
        res["excess_" + k] = res["pre_norm"][k] - res["post_norm"][k]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    brief = {k: v for k, v in res.items() if k.startswith("excess_")}
    for n in models:
        brief[n] = {k: res[n][k] for k in ("forward_ms", "backbone_ms", "encoder_ms", "decoder_ms", "launches")}
        brief[n]["spread"] = {k: res[n][k + "_spread"] for k in ("forward_ms", "encoder_ms", "decoder_ms")}
        brief[n]["per_kind"] = {k: [v["launches"], round(v["ms"], 4)] for k, v in res[n]["per_kind"].items()
                                if ".enc" in k or ".dec" in k or k.startswith("dec.") or k in ("heads", "gemm.dec")}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
