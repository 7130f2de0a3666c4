"""Golden-vector generator for the DETR keypoint model behind the reference's plain backbone
(`--backbone resnet50`: REV/models/backbone.py:57-102,188-190; REV/train_backbone.sh:10-21 "resnet50s16").
Runs ONLY where the reference checkout exists (the build machine); the test-suite reads what it wrote.

The reference's own model code is imported through oracle/gen_golden.py's helpers and the torchvision shim
(oracle/tvshim); build_model runs with backbone="resnet50" on spe.synthetic's seeded weights and crops.
Only numbers and key names are written:

  tests/golden/model_r50s16_<tag>.npz : the fields of the other model_*.npz records (config, seeds, input
      checksum, pred_logits / pred_points, aux layers, hs, PostProcess outputs, clip boxes) with the stage
      checksums of this model: chk_xs16 (the body's output), chk_src (input_proj's) and chk_memory.
      `cond_points_f64_vs_f32`: the conditioning value below.  No weights are stored.
  tests/golden/model_keys_r50s16.json : the reference state_dict's key names and shapes at 2/2 and 3/3 layers.

Conditioning: seeded random weights can amplify rounding.  Before a case is written, tests/model_s16_ref.py
runs in float64 and in float32 on the CPU; the seeds are kept only if their pred_points differ by at most
COND_MAX = 2e-5, a fifth of the 1e-4 parity contract, so the fixture leaves room for an fp32 implementation.
Otherwise the next weight seed is tried.  The measured value is printed and stored.

Usage: python tools/gen_golden_s16.py [tag ...]
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in ("satellite-pose-estimation_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))

import gen_golden as gg  # noqa: E402
from spe.config import SpeConfig  # noqa: E402
from spe.synthetic import random_weights, synthetic_batch  # noqa: E402

COND_MAX = 2e-5
CASES = {
    # tag: (cfg, batch, first weight seed, image seed)
    "s128_q11_l2": (SpeConfig(input_size=128, num_queries=11, enc_layers=2, dec_layers=2, backbone="resnet50"), 2, 29, 31),
    "s224_q30_l2": (SpeConfig(input_size=224, num_queries=30, enc_layers=2, dec_layers=2, backbone="resnet50"), 1, 37, 41),
    # REV/train_backbone.sh:10-21: --backbone resnet50 --input_size 448 --num_queries 40, 3/3 layers
    "s448_q40_l3": (SpeConfig(input_size=448, num_queries=40, enc_layers=3, dec_layers=3, backbone="resnet50"), 1, 43, 47),
}


def _args(cfg):
    a = gg._args(cfg)
    a.backbone = cfg.backbone
    return a


def _keys(model):
    return [[k, list(v.shape)] for k, v in model.state_dict().items() if not k.endswith("num_batches_tracked")]


def conditioning(cfg, w, images):
    import torch
    import model_s16_ref
    with torch.no_grad():
        p64 = model_s16_ref.forward(images, w, cfg, dtype=torch.float64)["pred_points"]
        p32 = model_s16_ref.forward(images, w, cfg)["pred_points"]
    return float((p64 - p32.double()).abs().max())


def main():
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    build_model, PostProcess = gg._import_reference()
    out_dir = os.path.join(REPO, "tests", "golden")
    only = set(sys.argv[1:])
    keys = {}
    for tag, (cfg, B, wseed0, iseed) in CASES.items():
        if only and tag not in only:
            continue
        model, _, _ = build_model(_args(cfg))
        model.eval()
        kl = _keys(model)
        assert not any(k.startswith(("backbone.0.body.layer4", "backbone.0.body.fc", "backbone.0.s8_latern",
                                     "backbone.0.s16_latern", "backbone.0.output_conv")) for k, _ in kl)
        keys[f"l{cfg.enc_layers}"] = kl
        batch = synthetic_batch(cfg, B, iseed)
        for wseed in range(wseed0, wseed0 + 8):
            w = random_weights(cfg, wseed)
            cond = conditioning(cfg, w, batch["images"])
            print(f"{tag}: weight seed {wseed}: pred_points fp64 vs fp32 {cond:.3e} (kept if <= {COND_MAX:g})")
            if cond <= COND_MAX:
                break
        else:
            raise SystemExit(f"{tag}: no well-conditioned weight seed in [{wseed0}, {wseed0 + 8})")
        model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        stages = {}
        model.backbone[0].body.register_forward_hook(lambda m, i, o: stages.update(xs16=o["0"].detach()))
        model.input_proj.register_forward_hook(lambda m, i, o: stages.update(src=o.detach()))
        model.transformer.register_forward_hook(lambda m, i, o: stages.update(memory=o[1].detach(), hs=o[0].detach()))
        with torch.no_grad():
            out = model(torch.from_numpy(batch["images"]))
        S = cfg.input_size
        assert tuple(stages["xs16"].shape) == (B, 1024, S // 16, S // 16)
        clip = [torch.as_tensor(b) for b in batch["clip_bbox"]]
        # (PostProcess rescales its CPU copy in place: hand it clones, as oracle/gen_golden.py does)
        out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}
        pp = PostProcess()({"pred_logits": out["pred_logits"].clone(), "pred_points": out["pred_points"].clone()}, clip)
        rec = {
            "config": json.dumps(cfg.to_dict()), "batch": B, "weight_seed": wseed, "image_seed": iseed,
            "input_checksum": gg._chk(batch["images"]),
            "pred_logits": out["pred_logits"].numpy(), "pred_points": out["pred_points"].numpy(),
            "aux_logits": np.stack([a["pred_logits"].numpy() for a in out["aux_outputs"]]),
            "aux_points": np.stack([a["pred_points"].numpy() for a in out["aux_outputs"]]),
            "hs": stages["hs"].numpy(),
            "pp_probs": np.stack([r["logits"] for r in pp]), "pp_points": np.stack([r["points"] for r in pp]),
            "clip_bbox": batch["clip_bbox"],
            "cond_points_f64_vs_f32": cond,
        }
        for k in ("xs16", "src", "memory"):
            rec["chk_" + k] = gg._chk(stages[k].numpy())
        path = os.path.join(out_dir, f"model_r50s16_{tag}.npz")
        np.savez_compressed(path, **rec)
        print("wrote", path, {k: np.asarray(v).shape for k, v in rec.items() if k != "config"})
    if not only:
        path = os.path.join(out_dir, "model_keys_r50s16.json")
        with open(path, "w") as f:
            json.dump(keys, f, indent=0)
            f.write("\n")
        print("wrote", path, {k: len(v) for k, v in keys.items()})


if __name__ == "__main__":
    main()
