"""MobileNetV3_Small RT-DETR, two measurements.

(default, CPU)  What bf16 storage costs, as tools/measure_bf16_rtdetr_mbv3.py measures it for Large: the torch
restatement (tests/rtdetr_mbv3s_ref.py) with every weight and every tensor a backbone kernel stores rounded to
bf16 -- at the fused entry's storage points and at the launch-per-layer path's --, the encoder / decoder weights
and the encoder outputs rounded, against the fp32 golden (tests/golden/rtdetr_mbv3s_s256.npz).

(--time, MI355X)  The fused entry kernel against the launch-per-layer block 0 (SPE_MBS_ENTRY=1 / 0, read once
per process: every sample is a fresh child process), bf16, B = 64: ms of the backbone stage and of the whole
forward, `--rounds` interleaved samples a path, each the median of `--iters` event-timed calls after a warm-up.
Prints one JSON document: the samples, the medians, the run-to-run spread of each path ((max - min) / median over
its samples) and the decision -- the fused entry is the default only if its median step beats the unfused one by
more than the larger spread.

Usage: python tools/measure_bf16_rtdetr_mbv3s.py [--time [--batch 64] [--rounds 3] [--iters 50]]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("satellite-pose-estimation_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))


def bf16_cost():
    import numpy as np
    import torch
    import rtdetr_ref
    import rtdetr_mbv3s_ref
    from test_rtdetr_mbv3s import reference_run
    r = reference_run()
    g, cfg = r["g"], r["cfg"]
    rnd = lambda t: t.to(torch.bfloat16).float()
    w16 = {k: rnd(torch.from_numpy(v)) if v.ndim >= 2 else torch.from_numpy(v) for k, v in r["w"].items()}
    x = torch.from_numpy(r["batch"]["images"])
    for fused in (True, False):
        with torch.no_grad():
            feats = rtdetr_mbv3s_ref.mobilenetv3_small_rounded(x, r["w"], rnd, fused=fused)
            print("fused entry" if fused else "launch per layer", "- backbone maps max |d| vs fp32:",
                  [(a - b).abs().max().item() for a, b in zip(feats, r["trace"]["feats"])])
            enc, _ = rtdetr_ref.hybrid_encoder(feats, w16, cfg)
            trace = {}
            o = rtdetr_ref.rtdetr_decoder([rnd(e) for e in enc], w16, cfg, trace)
        sel, ref_sel = trace["topk"].numpy(), g["topk_ind"]
        for b in range(sel.shape[0]):
            same = sel[b] == ref_sel[b]
            print(f"  image {b}: overlap {len(set(sel[b]) & set(ref_sel[b]))}/{cfg.num_queries}, same rank {int(same.sum())},",
                  "points", np.abs(o["pred_pts"][b].numpy()[same] - g["pred_pts"][b][same]).max(),
                  "logits", np.abs(o["pred_logits"][b].numpy()[same] - g["pred_logits"][b][same]).max())


def time_child(B, iters):
    """One sample in this process: median ms of the backbone stage and of the whole forward."""
    import torch
    from spe.rtdetr import RTDETR
    from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights
    cfg = RtdetrConfig(backbone="MobileNetV3_Small")
    m = RTDETR(cfg, "bf16")
    m.load_state_dict(random_rtdetr_weights(cfg, 0))
    dev = torch.device("cuda:0")
    x = torch.randn(B, 3, 256, 256, device=dev)
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

    print(json.dumps({"entry": int(os.environ.get("SPE_MBS_ENTRY", "1")), "backbone_ms": med(lambda: m.encode(x, ws, part="backbone")),
                      "step_ms": med(lambda: m(x, aux=False))}))


def time_ab(B, rounds, iters):
    samples = {"fused": [], "unfused": []}
    for _ in range(rounds):
        for name, knob in (("unfused", "0"), ("fused", "1")):
            env = dict(os.environ, SPE_MBS_ENTRY=knob)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--batch", str(B), "--iters", str(iters)],
                               env=env, capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                raise SystemExit(f"child failed ({name}): {r.stderr[-2000:]}")
            samples[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"batch": B, "dtype": "bf16", "iters": iters, "samples": samples}
    for key in ("backbone_ms", "step_ms"):
        for name in samples:
            v = [s[key] for s in samples[name]]
            out[f"{name}_{key}_median"] = statistics.median(v)
            out[f"{name}_{key}_spread"] = (max(v) - min(v)) / statistics.median(v)
    spread = max(out["fused_step_ms_spread"], out["unfused_step_ms_spread"])
    gain = 1.0 - out["fused_step_ms_median"] / out["unfused_step_ms_median"]
    out.update(step_gain=gain, step_spread=spread, fused_is_default=bool(gain > spread))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if a.child:
        time_child(a.batch, a.iters)
    elif a.time:
        time_ab(a.batch, a.rounds, a.iters)
    else:
        bf16_cost()
