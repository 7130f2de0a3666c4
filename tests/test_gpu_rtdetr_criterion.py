"""UNC RT-DETR set criterion on the device (spe_criterion_sigma, csrc/criterion_sigma.hip;
spe.rtdetr.SetCriterion) and spe.engine.evaluate_rtdetr, the GPU half.

Against the reference's goldens (tests/golden/rtdetr_criterion_<tag>.npz): matchings exact, losses
|d| <= 1e-5 * max(1, |v|) (the reference computes them in fp32).  Against the restatement
(tests/rtdetr_criterion_ref.py, itself pinned on those goldens by tests/test_rtdetr_criterion.py):
near-tie cost matrices, the shape limits, layers without a sigma, and the HIP model's own outputs;
same tolerance, matchings exact.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import rtdetr_criterion_ref as rr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TAGS = ["r18_s128", "r18_s256", "r50_s256"]
NAMES = ("loss_ce", "class_error", "cardinality_error", "loss_bbox_points", "loss_bbox_points_uncert", "points_different")


def close(got, want):
    return abs(got - want) <= 1e-5 * max(1.0, abs(want))


def to_device(outputs, dev):
    import torch
    f = lambda o: {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in o.items() if k != "aux_outputs"}
    d = f(outputs)
    d["aux_outputs"] = [f(a) for a in outputs["aux_outputs"]]
    return d


def device_targets(labels, points, dev):
    import torch
    return [{"labels": torch.from_numpy(labels[b]).to(dev), "landmarks": torch.from_numpy(points[b]).to(dev)}
            for b in range(len(labels))]


def call_entry(dev, logits, points, sigmas, flags, labels, tpts, cost_class=2.0, cost_bbox=5.0, sigmoid_cost=1,
               eos_coef=1e-4, shape=None, stream=None, out=None):
    """spe_criterion_sigma on numpy inputs -> (rc, match [L,B,T], losses [L,6]); `shape` overrides the
    (L, B, Q, C, T) the entry is told."""
    import torch
    from spe import _lib
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    lg, pt, sg = t(logits, torch.float32), t(points, torch.float32), t(sigmas, torch.float32)
    fl, lb, tp = t(np.asarray(flags), torch.int32), t(labels, torch.int32), t(tpts, torch.float32)
    L, B, Q, C = logits.shape
    T = labels.shape[1]
    if out is None:
        out = (torch.full((L, B, T), -7, dtype=torch.int32, device=dev),
               torch.full((L, 6), -7.0, dtype=torch.float64, device=dev))
    L, B, Q, C, T = shape or (L, B, Q, C, T)
    rc = _lib.lib().spe_criterion_sigma(_lib.stream_ptr(stream), _lib.ptr(lg), _lib.ptr(pt), _lib.ptr(sg), _lib.ptr(fl),
                                        _lib.ptr(lb), _lib.ptr(tp), L, B, Q, C, T, cost_class, cost_bbox, sigmoid_cost,
                                        eos_coef, float(B * T), _lib.ptr(out[0]), _lib.ptr(out[1]))
    torch.cuda.synchronize()
    return rc, out[0].cpu().numpy(), out[1].cpu().numpy()


def random_case(seed, L, B, Q, C, T, flags):
    rng = np.random.Generator(np.random.PCG64(seed))
    logits = rng.normal(0, 2, size=(L, B, Q, C)).astype(np.float32)
    points = rng.uniform(0, 1, size=(L, B, Q, 2)).astype(np.float32)
    sigmas = rng.normal(0, 1, size=(L, B, Q, 2)).astype(np.float32)
    labels = np.stack([rng.permutation(C - 1)[:T] for _ in range(B)]).astype(np.int64)
    tpts = rng.uniform(0, 1, size=(B, T, 2)).astype(np.float32)
    layers = [(logits[l], points[l], sigmas[l] if flags[l] else None) for l in range(L)]
    return logits, points, sigmas, labels, tpts, layers


@pytest.mark.parametrize("setting", rr.SETTINGS)
@pytest.mark.parametrize("tag", TAGS)
def test_hip_matches_reference(gpu_device, tag, setting):
    from spe.rtdetr import SetCriterion
    g = np.load(os.path.join(GOLDEN, f"rtdetr_{tag}.npz"))
    c = np.load(os.path.join(GOLDEN, f"rtdetr_criterion_{tag}.npz"))
    kw, ref, ref_match = rr.golden_setting(c, setting)
    crit = SetCriterion(**kw)
    losses = crit(to_device(rr.golden_outputs(g), gpu_device), device_targets(c["tgt_labels"], c["tgt_points"], gpu_device))
    assert np.array_equal(crit.last_match.cpu().numpy(), ref_match)
    assert set(losses) == set(ref)
    for k, v in ref.items():
        got = float(losses[k])
        print("deviation", tag, setting, k, got, v, abs(got - v))
        assert close(got, v), (k, got, v)


@pytest.mark.parametrize("sigmoid_cost", [1, 0])
def test_near_ties_match_restatement(gpu_device, sigmoid_cost):
    """Near-tie cost matrices: the queries' points are a few ulps apart, so an assignment flips on the
    last bit of cost_bbox * cp + cost_class * cc.  The logits are all 0, so sigmoid is exactly 0.5
    and softmax exactly 1/12 in every implementation; only the cost rounding decides, and
    criterion_sigma.hip is built without FMA contraction like the reference's separate torch ops."""
    rng = np.random.Generator(np.random.PCG64(78))
    B, Q, T, C = 64, 30, 11, 12
    base = rng.uniform(0.2, 0.8, size=(B, 1, 2)).astype(np.float32)
    pts = (base + rng.integers(-3, 4, size=(B, Q, 2)).astype(np.float32) * np.float32(6e-8)).astype(np.float32)
    logits = np.zeros((B, Q, C), np.float32)
    sig = rng.normal(0, 1, size=(B, Q, 2)).astype(np.float32)
    labels = np.stack([rng.permutation(C - 1)[:T] for _ in range(B)]).astype(np.int64)
    tpts = rng.uniform(0, 1, size=(B, T, 2)).astype(np.float32)
    _, match, raw = rr.criterion([(logits, pts, sig)], labels, tpts, use_focal_loss=bool(sigmoid_cost))
    rc, m, v = call_entry(gpu_device, logits[None], pts[None], sig[None], [1], labels, tpts, sigmoid_cost=sigmoid_cost)
    assert rc == 0
    assert np.array_equal(m, match)
    for i, k in enumerate(NAMES):
        assert close(v[0, i], raw[0][k]), (k, v[0, i], raw[0][k])


@pytest.mark.parametrize("case", ["q64_t32_c64", "q5_t5", "no_sigma_null", "sigma_off_in_the_middle"])
def test_shape_edges_match_restatement(gpu_device, case):
    L, B, Q, C, T, flags = {"q64_t32_c64": (2, 3, 64, 64, 32, [1, 0]), "q5_t5": (2, 3, 5, 12, 5, [1, 1]),
                            "no_sigma_null": (1, 3, 30, 12, 11, [0]),
                            "sigma_off_in_the_middle": (3, 2, 30, 12, 11, [1, 0, 1])}[case]
    logits, points, sigmas, labels, tpts, layers = random_case(len(case), L, B, Q, C, T, flags)
    for sigmoid_cost in (1, 0):
        _, match, raw = rr.criterion(layers, labels, tpts, use_focal_loss=bool(sigmoid_cost))
        rc, m, v = call_entry(gpu_device, logits, points, None if case == "no_sigma_null" else sigmas, flags, labels,
                              tpts, sigmoid_cost=sigmoid_cost)
        assert rc == 0
        assert np.array_equal(m, match)
        for l in range(L):
            for i, k in enumerate(NAMES):
                assert close(v[l, i], raw[l][k]), (l, k, v[l, i], raw[l][k])
            if not flags[l]:      # s = 0: the uncertainty form is the plain L1
                assert v[l, 4] == v[l, 3]


@pytest.mark.parametrize("case", ["q65", "t_gt_q", "c65", "t33"])
def test_unsupported_shapes_are_refused_before_any_launch(gpu_device, case):
    from spe import _lib
    Q, C, T = {"q65": (65, 12, 11), "t_gt_q": (5, 12, 6), "c65": (30, 65, 11), "t33": (64, 40, 33)}[case]
    logits, points, sigmas, labels, tpts, _ = random_case(3, 1, 2, Q, C, T, [1])
    rc, m, v = call_entry(gpu_device, logits, points, sigmas, [1], labels, tpts)
    assert rc == -1                                        # SPE_E_ARG
    assert b"bad argument" in _lib.lib().spe_last_error()
    assert (m == -7).all() and (v == -7.0).all()           # nothing ran


def test_unsupported_losses_raise():
    from spe.rtdetr import SetCriterion
    for bad in ("masks", "boxes", "vfl"):
        with pytest.raises(ValueError):
            SetCriterion(losses=("labels", bad))


_e2e = {}


def hip_outputs(dev):
    """The fp32 RTDETR at r18_s128 with the golden's weight and image seeds, aux on (built once)."""
    import torch
    from spe.config import SpeConfig
    from spe.rtdetr import RTDETR
    from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights
    from spe.synthetic import synthetic_batch
    if not _e2e:
        g = np.load(os.path.join(GOLDEN, "rtdetr_r18_s128.npz"))
        cfg = RtdetrConfig(**json.loads(str(g["config"])))
        m = RTDETR(cfg, "fp32", aux_outputs=True)
        m.load_state_dict(random_rtdetr_weights(cfg, int(g["weight_seed"])))
        b = synthetic_batch(SpeConfig(input_size=cfg.input_size), int(g["batch"]), int(g["image_seed"]))
        _e2e.update(model=m, cfg=cfg, images=torch.from_numpy(b["images"]).to(dev),
                    clip=torch.from_numpy(g["clip_bbox"]).float().to(dev))
    return _e2e


def test_criterion_on_hip_model_outputs(gpu_device):
    import torch
    from spe.rtdetr import build_rtdetr_criterion
    e = hip_outputs(gpu_device)
    c = np.load(os.path.join(GOLDEN, "rtdetr_criterion_r18_s128.npz"))
    o = e["model"](e["images"])
    crit = build_rtdetr_criterion(e["cfg"])
    assert crit.weight_dict == {"loss_ce": 1, "loss_bbox": 2}
    losses = crit(o, device_targets(c["tgt_labels"], c["tgt_points"], gpu_device))
    torch.cuda.synchronize()
    host = lambda d: {k: v.cpu().numpy() for k, v in d.items() if k.startswith("pred_")}
    layers = rr.layers_of({**host(o), "aux_outputs": [host(a) for a in o["aux_outputs"]]})
    assert len(layers) == e["cfg"].dec_layers + 1 and layers[-1][2] is None
    ref, match, _ = rr.criterion(layers, c["tgt_labels"], c["tgt_points"])
    assert np.array_equal(crit.last_match.cpu().numpy(), match)
    assert set(losses) == set(ref)
    for k, v in ref.items():
        assert close(float(losses[k]), v), (k, float(losses[k]), v)


def test_evaluate_rtdetr_on_synthetic_loader(gpu_device):
    import torch
    from spe.engine import evaluate_rtdetr
    from spe.rtdetr import RTDETRPostProcessor, build_rtdetr_criterion
    from spe.solver import SimplePoseSolverSigma
    e = hip_outputs(gpu_device)
    c = np.load(os.path.join(GOLDEN, "rtdetr_criterion_r18_s128.npz"))
    names = [f"img{i:06d}.jpg" for i in range(4)]
    gt = {n: {"quat": [1.0, 0.0, 0.0, 0.0], "tvec": [0.1 * i, -0.2, 8.0 + i]} for i, n in enumerate(names)}
    images = e["images"].cpu()
    loader = []
    for i in range(2):
        tg = [{"filename": names[2 * i + b], "clip_bbox": e["clip"][b].cpu(),
               "labels": torch.from_numpy(c["tgt_labels"][(b + i) % 2]), "landmarks": torch.from_numpy(c["tgt_points"][b])}
              for b in range(2)]
        loader.append((images.flip(0) if i else images, tg))
    crit = build_rtdetr_criterion(e["cfg"])
    seen = []

    class Recording:
        weight_dict = crit.weight_dict

        def __call__(self, outputs, targets):
            ld = crit(outputs, targets)
            seen.append({k: float(v) for k, v in ld.items()})
            return ld

    stats, ev = evaluate_rtdetr(e["model"], Recording(), {"bbox": RTDETRPostProcessor()}, loader, gt,
                                SimplePoseSolverSigma(), gpu_device)
    keys = ["class_error", "loss_ce", "loss_bbox"] + [f"{k}_aux_{i}" for i in range(3) for k in ("loss_ce", "loss_bbox")]
    assert len(seen) == 2 and set(seen[0]) == set(keys)
    want = {"loss", "class_error", "loss_ce", "loss_bbox", "speed_eval_pose"} | {k + "_unscaled" for k in keys}
    assert set(stats) == want
    wd = crit.weight_dict
    mean = lambda f: (f(seen[0]) + f(seen[1])) / 2
    assert stats["loss"] == mean(lambda d: d["loss_ce"] * wd["loss_ce"] + d["loss_bbox"] * wd["loss_bbox"])
    assert stats["loss_bbox"] == mean(lambda d: d["loss_bbox"] * wd["loss_bbox"])
    assert stats["class_error"] == mean(lambda d: d["class_error"])
    for k in keys:
        assert stats[k + "_unscaled"] == mean(lambda d: d[k])
    assert seen[0] != seen[1]
    assert list(ev.log) == names and stats["speed_eval_pose"] == ev.stats
    Q, C = e["cfg"].num_queries, e["cfg"].num_classes + 1
    for n in names:
        r = ev.log[n]
        assert {"points", "logits", "quat_pr", "tvec_pr", "score", "sigma", "aux_points_0", "aux_points_1",
                "aux_points_2"} <= set(r)
        assert np.asarray(r["sigma"]).shape == (Q, 2) and np.asarray(r["aux_points_2"]).shape == (Q, C)
    # aux_points_<i> are the aux entries' logits (the reference's naming), rounded to 2 decimals
    o = e["model"](e["images"], clip_bbox=e["clip"])
    want0 = np.around(o["aux_outputs"][0]["pred_logits"][1].cpu().numpy(), decimals=2)
    assert np.array_equal(np.asarray(ev.log[names[1]]["aux_points_0"], np.float32), want0.astype(np.float32))


def test_graph_capture_replays_identically(gpu_device):
    """One spe_criterion_sigma call captured into a graph (a single stream, no parallel branches)
    replays to the eager call's losses and matchings: the entry neither allocates nor synchronises
    once its per-stream scratch has the batch's size (the warm-up call on the capture stream)."""
    import torch
    from spe import _lib
    dev = gpu_device
    L, B, Q, C, T, flags = 3, 4, 30, 12, 11, [1, 1, 0]
    logits, points, sigmas, labels, tpts, _ = random_case(11, L, B, Q, C, T, flags)
    t = lambda a, dt: torch.from_numpy(a).to(dev, dt)
    lg, pt, sg = t(logits, torch.float32), t(points, torch.float32), t(sigmas, torch.float32)
    fl, lb, tp = t(np.asarray(flags), torch.int32), t(labels, torch.int32), t(tpts, torch.float32)
    match = torch.empty(L, B, T, dtype=torch.int32, device=dev)
    res = torch.empty(L, 6, dtype=torch.float64, device=dev)

    def run(stream):
        _lib.check(_lib.lib().spe_criterion_sigma(_lib.stream_ptr(stream), _lib.ptr(lg), _lib.ptr(pt), _lib.ptr(sg),
                                                  _lib.ptr(fl), _lib.ptr(lb), _lib.ptr(tp), L, B, Q, C, T, 2.0, 5.0, 1, 1e-4,
                                                  float(B * T), _lib.ptr(match), _lib.ptr(res)), "spe_criterion_sigma")

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(s)
    torch.cuda.synchronize()
    eager = (match.clone(), res.clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run(s)
    for _ in range(2):
        match.fill_(-1)
        res.fill_(-1.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(match, eager[0]) and torch.equal(res, eager[1])
    assert (eager[0] >= 0).all()
