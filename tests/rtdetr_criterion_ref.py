"""Restatement of the UNC RT-DETR set criterion in numpy (test infrastructure only).

  HungarianMatcher.forward    UNC/src/zoo/rtdetr/matcher.py:53-117: cost = cost_bbox * cdist_L1(
                              pred_pts, landmarks) + cost_class * (-prob[:, label]) with prob =
                              sigmoid(logits) under use_focal_loss, else softmax (fp32, torch's
                              order), then scipy's linear_sum_assignment per image (fp64;
                              oracle/criterion_ref.lsap, pinned against scipy in tests/test_criterion.py)
  SetCriterion.loss_labels    rtdetr_criterion.py:103-132: weighted cross entropy over every query
                              (matched -> its label, else no-object with weight eos_coef),
                              class_error = 100 - top-1 accuracy of the matched queries
  loss_cardinality            :134-148
  loss_points                 :150-174: sum |p - t| / num_boxes
  loss_points_uncert          :176-213: sum (|p - t| * exp(-s) + 0.5 * s) / num_boxes with s =
                              pred_sigmas, 0 for an entry without them; points_different = sum (p - t)
  forward                     :280-337: num_boxes the plain target count; the main output, then
                              aux_outputs as "<key>_aux_{i}"; every value multiplied by
                              weight_dict, other keys dropped except the main class_error

The per-element terms are fp32 like the reference's tensors, their sums fp64.
"""
from __future__ import annotations

import numpy as np

import criterion_ref as cr

LOSSES = ("labels", "cardinality", "points", "points_uncert")


def sigmoid32(x):
    x = np.asarray(x, np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


def match(logits, points, tgt_labels, tgt_points, cost_class=2.0, cost_bbox=5.0, sigmoid_cost=True, solver=cr.lsap):
    """One image: [T] query index matched to each target."""
    prob = sigmoid32(logits) if sigmoid_cost else cr.softmax32(logits)
    cc = -prob[:, tgt_labels]
    cp = np.abs(points[:, None, :].astype(np.float32) - tgt_points[None, :, :].astype(np.float32)).sum(-1, dtype=np.float32)
    C = (np.float32(cost_bbox) * cp + np.float32(cost_class) * cc).astype(np.float32)
    qi, ti = solver(C.astype(np.float64))
    out = np.full(len(tgt_labels), -1, np.int64)
    out[ti] = qi
    return out


def layer_values(logits, points, log_sigmas, tgt_labels, tgt_points, m, eos_coef, num_boxes):
    """The six unweighted values of one layer (spe_criterion_sigma's losses row); m [B, T]."""
    B, Q, C = logits.shape
    T = tgt_labels.shape[1]
    tc = np.full((B, Q), C - 1, np.int64)
    for b in range(B):
        tc[b, m[b]] = tgt_labels[b]
    lp = logits.astype(np.float64) - logits.max(-1, keepdims=True)
    lp = lp - np.log(np.exp(lp).sum(-1, keepdims=True))
    w = np.where(tc == C - 1, eos_coef, 1.0)
    nll = -np.take_along_axis(lp, tc[..., None], -1)[..., 0]
    pred = logits.argmax(-1)
    hit = np.concatenate([pred[b, m[b]] == tgt_labels[b] for b in range(B)])
    src = np.concatenate([points[b, m[b]] for b in range(B)]).astype(np.float32)
    tgt = np.concatenate([tgt_points[b] for b in range(B)]).astype(np.float32)
    s = (np.concatenate([log_sigmas[b, m[b]] for b in range(B)]).astype(np.float32) if log_sigmas is not None
         else np.zeros_like(src))
    d = src - tgt
    unc = np.abs(d) * np.exp(-s) + np.float32(0.5) * s
    return {"loss_ce": float((w * nll).sum() / w.sum()),
            "class_error": float(100.0 - 100.0 * hit.mean()),
            "cardinality_error": float(np.abs((pred != C - 1).sum(1) - T).mean()),
            "loss_bbox_points": float(np.abs(d).astype(np.float64).sum() / num_boxes),
            "loss_bbox_points_uncert": float(unc.astype(np.float64).sum() / num_boxes),
            "points_different": float(d.astype(np.float64).sum())}


def layers_of(outputs):
    """RTDETR.forward's dict (numpy) -> [(logits, points, log_sigmas or None)], main output first."""
    return [(o["pred_logits"], o["pred_pts"], o.get("pred_sigmas")) for o in [outputs] + list(outputs.get("aux_outputs", []))]


def criterion(layers, tgt_labels, tgt_points, matcher_weight_dict=None, weight_dict=None,
              losses=("labels", "points_uncert"), eos_coef=1e-4, use_focal_loss=True, solver=cr.lsap):
    """Returns (the reference's loss dict, match [L, B, T], the unweighted values per layer)."""
    mw = matcher_weight_dict or {"cost_class": 2, "cost_bbox": 5}
    wd = weight_dict or {"loss_ce": 1, "loss_bbox": 2}
    B, T = tgt_labels.shape
    out, ms, raw = {}, [], []
    for l, (lg, pt, sg) in enumerate(layers):
        m = np.stack([match(lg[b], pt[b], tgt_labels[b], tgt_points[b], mw["cost_class"], mw["cost_bbox"],
                            use_focal_loss, solver) for b in range(B)])
        ms.append(m)
        v = layer_values(lg, pt, sg, tgt_labels, tgt_points, m, eos_coef, float(B * T))
        raw.append(v)
        d = {}
        for name in losses:
            if name not in LOSSES:
                raise ValueError(name)
            if name == "labels":
                d["loss_ce"] = v["loss_ce"]
            elif name == "cardinality":
                d["cardinality_error"] = v["cardinality_error"]
            elif name == "points":
                d["loss_bbox"] = v["loss_bbox_points"]
            else:
                d["points_different"] = v["points_different"]
                d["loss_bbox"] = v["loss_bbox_points_uncert"]
        if l == 0 and "labels" in losses:
            out["class_error"] = v["class_error"]
        sfx = "" if l == 0 else f"_aux_{l - 1}"
        out.update({k + sfx: x * wd[k] for k, x in d.items() if k in wd})
    return out, np.stack(ms), raw


SETTINGS = ("sig_unc", "soft_unc", "sig_pts")     # scripts/gen_golden_rtdetr_criterion.py


def golden_outputs(g):
    """tests/golden/rtdetr_<tag>.npz -> the dict RTDETR.forward returns (numpy)."""
    aux = [{"pred_logits": a, "pred_pts": p, "pred_sigmas": s}
           for a, p, s in zip(g["aux_logits"], g["aux_pts"], g["aux_sigmas"])]
    aux.append({"pred_logits": g["enc_topk_logits"], "pred_pts": g["enc_topk_bboxes"]})
    return {"pred_logits": g["pred_logits"], "pred_pts": g["pred_pts"], "pred_sigmas": g["pred_sigmas"], "aux_outputs": aux}


def golden_setting(c, name):
    """One setting of tests/golden/rtdetr_criterion_<tag>.npz -> (criterion keyword arguments, the
    reference's loss dict, its matchings [L,B,T])."""
    kw = {"matcher_weight_dict": {"cost_class": 2, "cost_bbox": 5},
          "weight_dict": dict(zip([str(k) for k in c[f"{name}_weight_names"]], c[f"{name}_weight_values"].tolist())),
          "losses": tuple(str(k) for k in c[f"{name}_losses"]), "eos_coef": 1e-4,
          "use_focal_loss": bool(c[f"{name}_sigmoid_cost"])}
    ref = dict(zip([str(k) for k in c[f"{name}_loss_names"]], c[f"{name}_loss_values"].tolist()))
    return kw, ref, c[f"{name}_match"]
