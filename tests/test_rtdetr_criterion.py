"""UNC RT-DETR set criterion (UNC/src/zoo/rtdetr/rtdetr_criterion.py, matcher.py) and
its evaluate loop (UNC/solver/speed_engine.py:123-202), the CPU half.

The restatement (tests/rtdetr_criterion_ref.py) against the reference's own SetCriterion outputs on
the reference model's outputs (tests/golden/rtdetr_criterion_<tag>.npz,
scripts/gen_golden_rtdetr_criterion.py): three tags x three settings (sigmoid cost + points_uncert,
softmax cost + points_uncert, sigmoid cost + labels / cardinality / points).  Matchings exact;
losses |d| <= 1e-5 * max(1, |v|), the tolerance of tests/test_criterion.py (the reference computes
them in fp32).  evaluate_rtdetr's stat arithmetic on a stub model, criterion and solver.
"""
import os

import numpy as np
import pytest

import rtdetr_criterion_ref as rr
from conftest import GOLDEN

TAGS = ["r18_s128", "r18_s256", "r50_s256"]


def load(tag):
    g = np.load(os.path.join(GOLDEN, f"rtdetr_{tag}.npz"))
    c = np.load(os.path.join(GOLDEN, f"rtdetr_criterion_{tag}.npz"))
    return rr.golden_outputs(g), c


@pytest.mark.parametrize("setting", rr.SETTINGS)
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_reference(tag, setting):
    outputs, c = load(tag)
    kw, ref, ref_match = rr.golden_setting(c, setting)
    losses, match, _ = rr.criterion(rr.layers_of(outputs), c["tgt_labels"], c["tgt_points"], **kw)
    assert np.array_equal(match, ref_match)
    assert set(losses) == set(ref)
    for k, v in ref.items():
        print(tag, setting, k, losses[k], v, abs(losses[k] - v))
        assert abs(losses[k] - v) <= 1e-5 * max(1.0, abs(v)), (k, losses[k], v)


def test_goldens_are_not_trivial():
    """The fixtures exercise what they are for: the two cost forms match differently somewhere, the
    layers match differently, and the sigma term moves loss_bbox (it goes negative)."""
    differs = 0
    for tag in TAGS:
        _, c = load(tag)
        a, b = c["sig_unc_match"], c["soft_unc_match"]
        differs += int(not np.array_equal(a, b))
        assert not np.array_equal(a[0], a[-1])
        assert np.array_equal(a, c["sig_pts_match"])
        assert sorted(c["tgt_labels"][0].tolist()) == list(range(11))
    assert differs > 0
    _, c = load("r18_s128")
    unc = dict(zip(c["sig_unc_loss_names"], c["sig_unc_loss_values"]))
    pts = dict(zip(c["sig_pts_loss_names"], c["sig_pts_loss_values"]))
    assert unc["loss_bbox"] != pts["loss_bbox"] and unc["loss_ce"] == pts["loss_ce"]


def test_evaluate_rtdetr_stats_on_stubs(monkeypatch):
    """The reference loop's logging (speed_engine.py:157-173) with no device: the criterion's values
    arrive already weighted, the loop weights the keys weight_dict names once more; "loss" sums
    those, "<k>_unscaled" keeps what the criterion returned, every meter is the mean over batches."""
    import torch
    from spe import engine

    B, Q, C = 2, 5, 12
    names = [f"img{i}.jpg" for i in range(2 * B)]
    gt = {n: {"quat": [1.0, 0.0, 0.0, 0.0], "tvec": [0.0, 0.0, 5.0 + i]} for i, n in enumerate(names)}
    rng = np.random.Generator(np.random.PCG64(5))
    batches, calls = [], {"solve": 0}
    for i in range(2):
        t = [{"filename": names[i * B + b], "clip_bbox": torch.tensor([0.0, 0.0, 10.0, 10.0]),
              "labels": torch.arange(3), "landmarks": torch.zeros(3, 2)} for b in range(B)]
        batches.append((torch.zeros(B, 3, 8, 8), t))
    per_batch = [{"class_error": 50.0, "loss_ce": 1.5, "loss_bbox": 0.25, "loss_ce_aux_0": 2.0, "loss_bbox_aux_0": -0.5},
                 {"class_error": 25.0, "loss_ce": 0.5, "loss_bbox": 0.75, "loss_ce_aux_0": 1.0, "loss_bbox_aux_0": 0.125}]

    def model(samples, clip_bbox=None):
        assert clip_bbox is not None and clip_bbox.shape == (B, 4)
        f = lambda *s: torch.from_numpy(rng.normal(size=s).astype(np.float32))
        return {"pred_logits": f(B, Q, C), "pred_pts": f(B, Q, 2), "pred_sigmas": f(B, Q, 2),
                "probs": f(B, Q, C), "points_px": f(B, Q, 2), "sigmas": f(B, Q, 2).abs(),
                "aux_outputs": [{"pred_logits": f(B, Q, C) + k, "pred_pts": f(B, Q, 2)} for k in range(4)]}

    class Criterion:
        weight_dict = {"loss_ce": 1, "loss_bbox": 5}
        n = 0

        def __call__(self, outputs, targets):
            assert set(targets[0]) == {"clip_bbox", "labels", "landmarks"}
            d = per_batch[self.n]
            self.n += 1
            return {k: torch.tensor(v, dtype=torch.float64) for k, v in d.items()}

    class Solver:
        def solve_batch(self, points_px, probs, sigmas):
            calls["solve"] += 1
            assert sigmas is not None
            n = points_px.shape[0]
            return {"quat": torch.tensor([[1.0, 0, 0, 0]] * n), "tvec": torch.tensor([[0.0, 0, 5.0]] * n, dtype=torch.float64),
                    "status": torch.zeros(n, dtype=torch.int32)}

    monkeypatch.setattr(engine, "device_speed_score",
                        lambda q, t, qg, tg: (torch.linalg.norm(t - tg, dim=1) / torch.linalg.norm(tg, dim=1),
                                              torch.zeros(len(q), dtype=torch.float64)))
    stats, ev = engine.evaluate_rtdetr(model, Criterion(), None, batches, gt, Solver(), torch.device("cpu"))
    assert calls["solve"] == 2
    wd = Criterion.weight_dict
    want = {"class_error": 37.5, "speed_eval_pose": ev.stats,
            "loss": np.mean([d["loss_ce"] * wd["loss_ce"] + d["loss_bbox"] * wd["loss_bbox"] for d in per_batch])}
    for k in per_batch[0]:
        want[k + "_unscaled"] = np.mean([d[k] for d in per_batch])
        if k in wd:
            want[k] = np.mean([d[k] * wd[k] for d in per_batch])
    assert set(stats) == set(want)
    for k, v in want.items():
        assert stats[k] == v, (k, stats[k], v)
    assert list(ev.log) == names
    e = ev.log[names[0]]
    assert {"aux_points_0", "aux_points_1", "aux_points_2", "sigma"} <= set(e) and "aux_points_3" not in e
    assert "reliable" not in e and np.asarray(e["aux_points_1"]).shape == (Q, C)
    assert e["score_tvec"] == 0.0 and ev.log[names[1]]["score_tvec"] == round(1.0 / 6.0, 8)


def test_speed_eval_update_batch_unchanged_without_aux():
    """SpeedEval.update_batch's records for the existing callers carry no aux_points fields."""
    import torch
    from spe.speed_eval import SpeedEval
    ev = SpeedEval({"a.jpg": {"quat": [1.0, 0, 0, 0], "tvec": [0.0, 0, 5.0]}}, None)
    poses = {"quat": torch.tensor([[1.0, 0, 0, 0]]), "tvec": torch.tensor([[0.0, 0, 5.0]], dtype=torch.float64)}
    ev.update_batch(["a.jpg"], torch.zeros(1, 3, 2), torch.zeros(1, 3, 12), poses)
    assert set(ev.log["a.jpg"]) == {"points", "logits", "quat_gt", "tvec_gt", "quat_pr", "tvec_pr", "score_tvec",
                                    "score_quat", "score"}
