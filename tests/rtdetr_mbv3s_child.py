"""Child process of tests/test_gpu_rtdetr_mbv3s.py and tools/measure_bf16_rtdetr_mbv3s.py: the library reads
SPE_MBS_ENTRY once per process, so each path of the MobileNetV3_Small entry (fused kernel / launch by launch)
is run in a process of its own.  Runs the golden's weights and images through the fp32 and the bf16 model and
writes the backbone maps and the forward outputs to the .npz named on the command line.

Usage: SPE_MBS_ENTRY=0|1 python tests/rtdetr_mbv3s_child.py OUT.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "satellite-pose-estimation_amd"), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(out_path):
    from spe.rtdetr import RTDETR
    from test_rtdetr_mbv3s import golden
    from spe.config import SpeConfig
    from spe.rtdetr_spec import random_rtdetr_weights
    from spe.synthetic import synthetic_batch
    g, cfg = golden()
    w = random_rtdetr_weights(cfg, int(g["weight_seed"]))
    b = synthetic_batch(SpeConfig(input_size=cfg.input_size), int(g["batch"]), int(g["image_seed"]))
    dev = torch.device("cuda:0")
    x = torch.from_numpy(b["images"]).to(dev)
    clip = torch.from_numpy(g["clip_bbox"]).float().to(dev)
    rec = {"entry": np.int64(int(os.environ.get("SPE_MBS_ENTRY", "1")))}
    for dtype in ("fp32", "bf16"):
        m = RTDETR(cfg, dtype)
        m.load_state_dict(w)
        for i, f in enumerate(m.backbone_features(x)):
            rec[f"{dtype}_feat{i}"] = f.cpu().numpy()
        o = m(x, clip_bbox=clip)
        torch.cuda.synchronize()
        for k in ("pred_logits", "pred_pts", "pred_sigmas", "topk", "points_px", "probs", "sigmas"):
            rec[f"{dtype}_{k}"] = o[k].cpu().numpy()
        aux = o["aux_outputs"]
        for k in ("pred_logits", "pred_pts", "pred_sigmas"):
            rec[f"{dtype}_aux_{k}"] = np.stack([a[k].cpu().numpy() for a in aux[:-1]])
        rec[f"{dtype}_enc_logits"] = aux[-1]["pred_logits"].cpu().numpy()
        rec[f"{dtype}_enc_pts"] = aux[-1]["pred_pts"].cpu().numpy()
    np.savez(out_path, **rec)


if __name__ == "__main__":
    main(sys.argv[1])
