"""Golden-vector generator for the UNC RT-DETR set criterion.  Runs only where a
checkout of the reference exists; no test reads the reference, only the fixtures this writes.

Loads the reference's own UNC/src/zoo/rtdetr/{matcher,rtdetr_criterion,real_nvp}.py the way
oracle/gen_golden_rtdetr.py loads the model files: oracle/tvshim on sys.path for the torchvision
import, `src.core.register` as an identity decorator, `src.misc.dist` with the two functions the
criterion imports, and an empty `box_ops` (box losses the speed configs never run).  No reference
code is copied; only numbers are written.

The reference criterion is fed the committed reference model outputs (tests/golden/rtdetr_<tag>.npz:
the main output, the aux decoder layers, the encoder top-k entry without sigmas) as predictions,
with seeded targets: per image the labels are a permutation of 0..10, the landmarks uniform in
[0, 1) as fp32, and half of them moved to a main-output prediction plus small noise so that the
matchings are not trivial.  Three settings:

  sig_unc   use_focal_loss (sigmoid cost), losses labels + points_uncert, the speed config's weights
  soft_unc  softmax cost, losses labels + points_uncert, points_different kept through weight 1
  sig_pts   sigmoid cost, losses labels + cardinality + points, cardinality_error kept through weight 1

Writes tests/golden/rtdetr_criterion_<tag>.npz:
  tgt_labels [B,T] int64, tgt_points [B,T,2] fp32
  per setting s: <s>_sigmoid_cost, <s>_losses (names), <s>_weight_names / <s>_weight_values,
  <s>_loss_names / <s>_loss_values (fp64, what SetCriterion.forward returned), <s>_match [L,B,T]
  (query matched to each target, recorded by wrapping HungarianMatcher.forward; layer 0 = main output)
Usage: python scripts/gen_golden_rtdetr_criterion.py --reference <path to the reference checkout>
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
UNC_DIR = "Monocular Satellite Pose Estimation Based on Uncertainty Estimation and Self-Assessment"
TAGS = {"r18_s128": 31, "r18_s256": 32, "r50_s256": 33}      # tag: target seed


def _load(name, path, pkg):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    m.__package__ = pkg
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def import_reference(unc):
    sys.path.insert(0, os.path.join(REPO, "oracle", "tvshim"))
    core = types.ModuleType("src.core")
    core.register = lambda cls: cls
    dist = types.ModuleType("src.misc.dist")
    dist.get_world_size = lambda: 1
    dist.is_dist_available_and_initialized = lambda: False
    misc = types.ModuleType("src.misc")
    misc.__path__ = []
    misc.dist = dist
    src = types.ModuleType("src")
    src.__path__ = []
    src.core, src.misc = core, misc
    sys.modules.update({"src": src, "src.core": core, "src.misc": misc, "src.misc.dist": dist})
    zoo = os.path.join(unc, "src", "zoo", "rtdetr")
    pkg = types.ModuleType("unc_rtdetr_crit")
    pkg.__path__ = [zoo]
    sys.modules["unc_rtdetr_crit"] = pkg
    box_ops = types.ModuleType("unc_rtdetr_crit.box_ops")
    box_ops.box_cxcywh_to_xyxy = box_ops.box_iou = box_ops.generalized_box_iou = None
    sys.modules["unc_rtdetr_crit.box_ops"] = box_ops
    _load("unc_rtdetr_crit.real_nvp", os.path.join(zoo, "real_nvp.py"), "unc_rtdetr_crit")
    mt = _load("unc_rtdetr_crit.matcher", os.path.join(zoo, "matcher.py"), "unc_rtdetr_crit")
    cr = _load("unc_rtdetr_crit.rtdetr_criterion", os.path.join(zoo, "rtdetr_criterion.py"), "unc_rtdetr_crit")
    return mt, cr


def make_targets(g, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    B, Q, _ = g["pred_pts"].shape
    T = 11
    labels = np.stack([rng.permutation(T) for _ in range(B)]).astype(np.int64)
    pts = rng.uniform(0, 1, size=(B, T, 2)).astype(np.float32)
    for b in range(B):
        near = rng.permutation(T)[: T // 2]
        qs = rng.permutation(Q)[: T // 2]
        pts[b, near] = g["pred_pts"][b, qs] + rng.normal(0, 0.01, size=(T // 2, 2)).astype(np.float32)
    return labels, pts.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    import torch
    mt, cr = import_reference(os.path.join(os.path.abspath(args.reference), UNC_DIR))
    for tag, seed in TAGS.items():
        g = np.load(os.path.join(REPO, "tests", "golden", f"rtdetr_{tag}.npz"))
        depth = json.loads(str(g["config"]))["depth"]
        bbox_w = 5 if depth == 50 else 2
        settings = {
            "sig_unc": (True, ["labels", "points_uncert"], {"loss_ce": 1, "loss_bbox": bbox_w}),
            "soft_unc": (False, ["labels", "points_uncert"], {"loss_ce": 1, "loss_bbox": bbox_w, "points_different": 1}),
            "sig_pts": (True, ["labels", "cardinality", "points"], {"loss_ce": 1, "loss_bbox": bbox_w, "cardinality_error": 1}),
        }
        labels, pts = make_targets(g, seed)
        t = torch.from_numpy
        outputs = {"pred_logits": t(g["pred_logits"]), "pred_pts": t(g["pred_pts"]), "pred_sigmas": t(g["pred_sigmas"]),
                   "aux_outputs": [{"pred_logits": t(a), "pred_pts": t(p), "pred_sigmas": t(s)}
                                   for a, p, s in zip(g["aux_logits"], g["aux_pts"], g["aux_sigmas"])]
                   + [{"pred_logits": t(g["enc_topk_logits"]), "pred_pts": t(g["enc_topk_bboxes"])}]}
        targets = [{"labels": t(labels[b]), "landmarks": t(pts[b])} for b in range(labels.shape[0])]
        rec = {"tgt_labels": labels, "tgt_points": pts}
        for name, (focal, losses, wd) in settings.items():
            matcher = mt.HungarianMatcher({"cost_class": 2, "cost_bbox": 5, "cost_giou": 2}, use_focal_loss=focal)
            matches = []
            inner = matcher.forward

            def spy(o, tg, inner=inner, matches=matches):
                ind = inner(o, tg)
                m = np.full((len(tg), labels.shape[1]), -1, np.int64)
                for b, (i, j) in enumerate(ind):
                    m[b, j.numpy()] = i.numpy()
                matches.append(m)
                return ind
            matcher.forward = spy
            crit = cr.SetCriterion(matcher, wd, losses, eos_coef=1e-4, num_classes=11).eval()
            with torch.no_grad():
                ld = crit(outputs, targets)
            rec[f"{name}_sigmoid_cost"] = np.int64(focal)
            rec[f"{name}_losses"] = np.asarray(losses)
            rec[f"{name}_weight_names"] = np.asarray(list(wd))
            rec[f"{name}_weight_values"] = np.asarray(list(wd.values()), np.float64)
            rec[f"{name}_loss_names"] = np.asarray(list(ld))
            rec[f"{name}_loss_values"] = np.asarray([float(v) for v in ld.values()], np.float64)
            rec[f"{name}_match"] = np.stack(matches)
        path = os.path.join(REPO, "tests", "golden", f"rtdetr_criterion_{tag}.npz")
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes;", {k: len(rec[f"{k}_loss_names"]) for k in settings})


if __name__ == "__main__":
    main()
