"""The reference's backbone pair on the MI355X (REV/train_backbone.sh, REV/get_backbone_time.sh): the plain
ResNet-50 at stride 16 on 448 x 448 crops ("resnet50") against the stride-8 fusion neck on 224 x 224 crops
("resnet50s8"), 40 queries, 3 / 3 layers, at B = 25 (the reference's batch size) and B = 64, in bf16 and
fp32h3: model-forward images / s and the backbone stage alone (images -> src).  For the bf16 stride-16 model
also the A/B of the fused final tail (btail_wide.hip's final form: the last bottleneck's conv3 + identity +
relu + input_proj in one launch) against its two GEMMs, SPE_BTAIL_PROJ=1 against =0.

    python tools/measure_backbone_stride.py [--out profiles/backbone_s16_vs_s8.json]

Every case runs in a child process of its own (the knob is read once per process), one after the other; the
A/B cases alternate 0, 1, 0, 1 so that drift hits both sides.  Each sample is the median of `--iters` timed
calls after `--warmup` untimed ones, timed with device events around one call.  Random weights: the time
does not depend on their values.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "satellite-pose-estimation_amd"))

PAIR = {"resnet50": 448, "resnet50s8": 224}      # backbone -> input size (REV/train_backbone.sh:10-34)


def worker(case, warmup, iters):
    import torch

    from spe.config import SpeConfig
    from spe.models import DETR
    from spe.synthetic import random_weights, synthetic_batch
    dev = torch.device("cuda:0")
    cfg = SpeConfig(input_size=PAIR[case["backbone"]], num_queries=40, enc_layers=3, dec_layers=3,
                    backbone=case["backbone"])
    B = case["batch"]
    m = DETR(cfg, dtype=case["dtype"])
    m.load_state_dict(random_weights(cfg, 0))
    one = torch.from_numpy(synthetic_batch(cfg, 4, 1)["images"]).to(dev)
    img = one.repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous()
    ws = m.workspace(B, dev)

    def time_ms(fn):
        for _ in range(warmup):
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
        return statistics.median(ts), min(ts), max(ts)

    fwd = time_ms(lambda: m(img))
    bb = time_ms(lambda: m.encode(img, ws, part="backbone"))
    print(json.dumps({**case, "input_size": cfg.input_size, "tokens": cfg.tokens, "forward_ms": fwd[0],
                      "forward_ms_min_max": fwd[1:], "forward_img_per_s": B / (fwd[0] * 1e-3),
                      "backbone_stage_ms": bb[0], "backbone_stage_ms_min_max": bb[1:],
                      "backbone_img_per_s": B / (bb[0] * 1e-3), "SPE_BTAIL_PROJ": os.environ.get("SPE_BTAIL_PROJ", "1")}))


def run_case(case, args, knob=None):
    env = dict(os.environ)
    if knob is not None:
        env["SPE_BTAIL_PROJ"] = str(knob)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(case), "--warmup",
                          str(args.warmup), "--iters", str(args.iters)], env=env, capture_output=True, text=True,
                         timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"case {case} failed ({out.returncode}):\n{out.stdout}\n{out.stderr}")
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "backbone_s16_vs_s8.json"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=21)
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--worker")
    args = ap.parse_args()
    if args.worker:
        return worker(json.loads(args.worker), args.warmup, args.iters)
    import torch
    res = {"device": torch.cuda.get_device_name(0), "queries": 40, "layers": "3/3", "warmup": args.warmup,
           "iters": args.iters, "pair": [], "final_tail_ab": []}
    for B in (25, 64):
        for dtype in ("bf16", "fp32h3"):
            for bb in ("resnet50", "resnet50s8"):
                res["pair"].append(run_case({"backbone": bb, "batch": B, "dtype": dtype}, args))
    # the fused final tail against its two GEMMs (bf16, stride 16): alternating child processes
    for B in (25, 64):
        case = {"backbone": "resnet50", "batch": B, "dtype": "bf16"}
        runs = {0: [], 1: []}
        for _ in range(args.ab_rounds):
            for knob in (0, 1):
                runs[knob].append(run_case(case, args, knob))
        ab = {"batch": B, "rows": B * 28 * 28, "row_tiles_of_192": (B * 28 * 28 + 191) // 192}
        for knob in (0, 1):
            for k in ("forward_ms", "backbone_stage_ms"):
                v = [r[k] for r in runs[knob]]
                ab[f"{k}_proj{knob}"] = statistics.median(v)
                ab[f"{k}_proj{knob}_samples"] = v
        ab["backbone_stage_ms_saved"] = ab["backbone_stage_ms_proj0"] - ab["backbone_stage_ms_proj1"]
        res["final_tail_ab"].append(ab)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
