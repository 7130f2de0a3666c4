"""What bf16 storage costs the GhostNetV2 RT-DETR, measured on the CPU: the torch restatement
(tests/rtdetr_ghostv2_ref.py) with every weight a backbone MFMA kernel reads and every tensor a backbone kernel stores rounded to bf16, the
encoder / decoder weights rounded and the encoder outputs rounded, against the fp32 golden
(tests/golden/rtdetr_ghostv2_s256.npz).  The bf16 gates of tests/test_gpu_rtdetr_ghostv2.py are twice the printed
figures.

Usage: python tools/measure_bf16_rtdetr_ghostv2.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("satellite-pose-estimation_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))

import rtdetr_ref  # noqa: E402
import rtdetr_ghostv2_ref  # noqa: E402
from test_rtdetr_ghostv2 import reference_run  # noqa: E402


def main():
    r = reference_run()
    g, cfg = r["g"], r["cfg"]
    rnd = lambda t: t.to(torch.bfloat16).float()
    w16 = {k: rnd(torch.from_numpy(v)) if v.ndim >= 2 else torch.from_numpy(v) for k, v in r["w"].items()}
    x = torch.from_numpy(r["batch"]["images"])
    with torch.no_grad():
        feats = rtdetr_ghostv2_ref.ghostnetv2_rounded(x, r["w"], rnd)
        print("backbone maps max |d| vs fp32:", [(a - b).abs().max().item() for a, b in zip(feats, r["trace"]["feats"])])
        enc, _ = rtdetr_ref.hybrid_encoder(feats, w16, cfg)
        trace = {}
        o = rtdetr_ref.rtdetr_decoder([rnd(e) for e in enc], w16, cfg, trace)
    sel, ref_sel = trace["topk"].numpy(), g["topk_ind"]
    for b in range(sel.shape[0]):
        same = sel[b] == ref_sel[b]
        print(f"image {b}: overlap {len(set(sel[b]) & set(ref_sel[b]))}/{cfg.num_queries}, same rank {int(same.sum())},",
              "points", np.abs(o["pred_pts"][b].numpy()[same] - g["pred_pts"][b][same]).max(),
              "logits", np.abs(o["pred_logits"][b].numpy()[same] - g["pred_logits"][b][same]).max())


if __name__ == "__main__":
    main()
