"""GPU: the exhaustive four-point-subset solver (spe_pnp_exhaustive, ExhaustivePoseSolver) against its
numpy restatement (tests/pnp_exhaustive_ref.py), on the smallest shapes that can go wrong, on concurrent
streams, under batch permutation and through PosePipeline.

Tolerances: status, n_corr, corr_label, cand_index, inlier_mask and repro_final exact; poses |dq| <= 1e-5
and relative dt <= 1e-6 (test_solver_matches_oracle's bounds: the quaternion is float32, the device LM
solves its 6x6 step by Cholesky where the oracle takes a pseudo-inverse).  An image may be left out only
when, in the restatement's own error table, the K-th and (K+1)-th errors differ by less than 1e-6
relative; at most 2 % of the batch.  Everything else is bit-identity between device runs."""
import argparse
import functools

import numpy as np
import pytest
import torch

import pnp_exhaustive_ref as X
import pnp_ref
from helpers import solver_stress_set
from spe.config import Camera, SpeConfig, world_points
from spe.solver import ExhaustivePoseSolver, build_solver
from spe.synthetic import bench_weights, synthetic_batch

pytestmark = pytest.mark.gpu

K = Camera.K
W = world_points()
STRESS_SEED = 0           # tests/test_pnp_exhaustive.py checks its near-tie count on the CPU
FIELDS = ("status", "n_corr", "corr_label", "cand_index", "inlier_mask", "repro_final", "quat", "tvec", "rvec")


@functools.lru_cache(maxsize=None)
def _stress():
    return solver_stress_set(96, STRESS_SEED)


@functools.lru_cache(maxsize=None)
def _thresholds():
    """One get_repro_th threshold per image from seeded box areas: 1.5 (the growth path) up to 20."""
    area = np.random.default_rng(5).uniform(10, 600, 96)
    return np.array([pnp_ref.repro_th(a, 256) for a in area], np.float32)


def _solve(dev, solver, pts, probs, sig=None, th=None, **kw):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    o = solver.solve_batch(t(pts), t(probs), t(sig), repro_per_image=t(th), **kw)
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in FIELDS}


def _check(h, o, topk, min_ok=0.0, max_out=0.02):
    B = len(o["status"])
    out = np.array([len(e) > 0 and bool(X.near_tie(e, topk)) for e in o["errors"]])
    print(f"topk={topk}: {int(out.sum())} of {B} images left out (K-th / (K+1)-th error within 1e-6)")
    assert out.sum() <= max_out * B
    keep = ~out
    for k in ("status", "n_corr", "corr_label", "cand_index"):
        np.testing.assert_array_equal(h[k][keep], o[k][keep], err_msg=k)
    np.testing.assert_array_equal(h["inlier_mask"].astype(np.uint32)[keep], o["inlier_mask"].astype(np.uint32)[keep])
    np.testing.assert_array_equal(h["repro_final"][keep], o["repro_final"][keep])
    ok = (o["status"] == 0) & keep
    assert ok.sum() >= min_ok * B
    if ok.any():
        dq = np.abs(np.abs((h["quat"].astype(np.float64) * o["quat"]).sum(1)) - 1)
        dt = np.linalg.norm(h["tvec"] - o["tvec"], axis=1) / np.maximum(np.linalg.norm(o["tvec"], axis=1), 1e-9)
        print(f"  max |dq| {dq[ok].max():.3g}, max rel dt {dt[ok].max():.3g} over {int(ok.sum())} poses")
        assert dq[ok].max() <= 1e-5
        assert dt[ok].max() <= 1e-6
    bad = (o["status"] != 0) & keep
    assert np.all(h["quat"][bad] == 0) and np.all(h["tvec"][bad] == 0) and np.all(h["rvec"][bad] == 0)
    assert np.all(h["cand_index"][bad] == -1)


# ------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("topk,with_sigma,per_image", [(1, False, False), (10, False, False), (10, True, False),
                                                       (10, False, True), (10, True, True), (64, True, False),
                                                       (64, False, True), (1, True, True)])
def test_matches_the_restatement(gpu_device, topk, with_sigma, per_image):
    pts, probs, _, _, sig = _stress()
    sig = sig if with_sigma else None
    th = _thresholds() if per_image else None
    h = _solve(gpu_device, ExhaustivePoseSolver(topk=topk), pts, probs, sig, th)
    o = X.solve_batch(pts, probs, sig, K, W, 20.0 if th is None else th, topk)
    if per_image:
        assert (o["repro_final"] != th).any()              # the growth path ran
    _check(h, o, topk, min_ok=0.8)


def test_topk_400_is_refused(gpu_device):
    with pytest.raises(ValueError, match="topk"):
        ExhaustivePoseSolver(topk=400)
    s = ExhaustivePoseSolver(topk=10)
    s.topk = 400                                           # past the constructor: the C side refuses
    pts, probs, _, _, _ = _stress()
    from spe._lib import SpeError
    with pytest.raises(SpeError, match="topk"):
        _solve(gpu_device, s, pts[:2], probs[:2])


def test_area_gives_the_per_image_thresholds(gpu_device):
    pts, probs, _, _, _ = _stress()
    area = np.random.default_rng(5).uniform(10, 600, 96)
    s = ExhaustivePoseSolver(topk=10)
    a = _solve(gpu_device, s, pts, probs, area=area.tolist())
    b = _solve(gpu_device, s, pts, probs, th=_thresholds())
    for k in FIELDS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ------------------------------------------------------------------------------------ small shapes
def _onehot(n, Q=11, C=12):
    p = np.full((Q, C), 0.01, np.float32)
    p[:, C - 1] = 0.89
    p[np.arange(n), np.arange(n)] = 0.95
    p[np.arange(n), C - 1] = 0.01
    return p


def test_batch_of_one(gpu_device):
    pts, probs, _, _, sig = _stress()
    b = int(np.flatnonzero((probs.argmax(2) != 11).sum(1) >= 8)[0])
    h = _solve(gpu_device, ExhaustivePoseSolver(topk=10), pts[b:b + 1], probs[b:b + 1], sig[b:b + 1])
    o = X.solve_batch(pts[b:b + 1], probs[b:b + 1], sig[b:b + 1], K, W, 20.0, 10)
    _check(h, o, 10, min_ok=1.0, max_out=0.0)


def test_ragged_subset_counts_in_one_batch(gpu_device):
    """n = 4, 5 and 11 in one batch: 1, 5 and 330 subsets, the grid sized for 330 each."""
    pts = np.zeros((3, 11, 2), np.float32)
    probs = np.stack([_onehot(n) for n in (4, 5, 11)])
    for b, n in enumerate((4, 5, 11)):
        _, img, _, _ = X.synthetic_case(20 + b, noise=1.0, nout=1 if n == 11 else 0, K=K, world=W)
        pts[b] = img
    for topk in (1, 10):
        h = _solve(gpu_device, ExhaustivePoseSolver(topk=topk), pts, probs)
        o = X.solve_batch(pts, probs, None, K, W, 20.0, topk)
        np.testing.assert_array_equal(o["n_corr"], [4, 5, 11])
        assert [len(e) for e in o["errors"]] == [1, 5, 330] and o["cand_index"][0] == 0
        _check(h, o, topk, min_ok=1.0, max_out=0.0)


def test_q30_with_duplicate_labels(gpu_device):
    pts, probs, _, _, sig = solver_stress_set(6, 31, Q=30)
    assert any(len(set(l.tolist()) - {11}) < (l != 11).sum() for l in probs.argmax(2))   # duplicates present
    h = _solve(gpu_device, ExhaustivePoseSolver(topk=10), pts, probs, sig)
    o = X.solve_batch(pts, probs, sig, K, W, 20.0, 10)
    _check(h, o, 10, min_ok=0.5, max_out=0.0)


def test_no_foreground_next_to_a_solvable_image(gpu_device):
    _, img, _, _ = X.synthetic_case(7, noise=0.5, K=K, world=W)
    pts = np.stack([np.zeros((11, 2), np.float32), img, img[::-1].copy()])
    probs = np.stack([_onehot(0), _onehot(11), _onehot(3)])
    h = _solve(gpu_device, ExhaustivePoseSolver(topk=10), pts, probs)
    o = X.solve_batch(pts, probs, None, K, W, 20.0, 10)
    np.testing.assert_array_equal(o["status"], [pnp_ref.ST_NO_FG, pnp_ref.ST_OK, pnp_ref.ST_CV_ERROR])
    _check(h, o, 10, max_out=0.0)
    np.testing.assert_array_equal(h["repro_final"], np.float32([20, 20, 20]))


# ------------------------------------------------------------------------------------ streams, batches
def test_solves_on_concurrent_streams(gpu_device):
    """Two different batches solved back to back on two streams, interleaved over several rounds: the
    hypothesis records are per (device, stream), so each result has the bits of the same batch alone."""
    dev = gpu_device
    sets = [solver_stress_set(48, seed=s) for s in (21, 22)]
    s = ExhaustivePoseSolver(topk=10)
    alone = [_solve(dev, s, p, r, g) for p, r, _, _, g in sets]
    ins = [tuple(torch.from_numpy(a).to(dev) for a in (p, r, g)) for p, r, _, _, g in sets]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    outs = []
    for _ in range(4):
        for (p, r, g), st in zip(ins, streams):
            with torch.cuda.stream(st):
                outs.append(s.solve_batch(p, r, g, stream=st))
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        for k in FIELDS:
            np.testing.assert_array_equal(o[k].cpu().numpy(), alone[i % 2][k], err_msg=f"{i} {k}")
    assert not np.array_equal(alone[0]["tvec"], alone[1]["tvec"])


def test_batch_permutation(gpu_device):
    pts, probs, _, _, sig = _stress()
    th = _thresholds()
    perm = np.random.default_rng(1).permutation(96)
    s = ExhaustivePoseSolver(topk=10)
    a = _solve(gpu_device, s, pts, probs, sig, th)
    b = _solve(gpu_device, s, pts[perm], probs[perm], sig[perm], th[perm])
    for k in FIELDS:
        np.testing.assert_array_equal(b[k], a[k][perm], err_msg=k)


# ------------------------------------------------------------------------------------ pipeline
def _pipeline_equals_solve_batch(dev, m, images, clip, solver, modes):
    from spe.pipeline import PosePipeline
    B = images.shape[0]
    n_ok = 0
    for kw in modes:
        p = PosePipeline(m, solver, B, device=dev, **kw)
        outs = []
        for _ in range(2):
            p.load(images, clip)
            outs.append(p.run())
        for o in outs:
            p.wait(o)
        torch.cuda.synchronize()
        for o in outs:
            fo = o["forward"]
            ref = solver.solve_batch(fo["points_px"], fo["probs"], fo.get("sigmas"))
            torch.cuda.synchronize()
            for k in FIELDS:
                assert torch.equal(o["poses"][k], ref[k]), (kw, k)
            n_ok += int((ref["status"] == 0).sum())
    return n_ok


def test_pipeline_with_a_small_detr(gpu_device):
    from spe.models import DETR
    cfg = SpeConfig(input_size=128, num_queries=11, enc_layers=2, dec_layers=2)

    def hs_fn(w, images):
        m = DETR(cfg, dtype="fp32")
        m.load_state_dict(w)
        return m(torch.from_numpy(images).to(gpu_device), return_hs=True)["hs"].cpu().numpy()

    m = DETR(cfg, dtype="fp32")
    m.load_state_dict(bench_weights(cfg, 3, hs_fn))
    b = synthetic_batch(cfg, 8, 41)
    solver = build_solver(argparse.Namespace(solver="exhaustive", topk=10))
    n_ok = _pipeline_equals_solve_batch(gpu_device, m, torch.from_numpy(b["images"]).to(gpu_device),
                                        torch.from_numpy(b["clip_bbox"]).float().to(gpu_device), solver,
                                        [{}, dict(overlap=True)])
    assert n_ok > 0


def test_pipeline_with_an_rtdetr_r18(gpu_device):
    from spe.rtdetr import RTDETR
    from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights
    cfg = RtdetrConfig(depth=18, input_size=128)
    m = RTDETR(cfg, dtype="bf16")
    m.load_state_dict(random_rtdetr_weights(cfg, 0))
    b = synthetic_batch(SpeConfig(input_size=128), 4, 42)
    solver = build_solver(argparse.Namespace(solver="exhaustive", topk=10))
    n_ok = _pipeline_equals_solve_batch(gpu_device, m, torch.from_numpy(b["images"]).to(gpu_device),
                                        torch.from_numpy(b["clip_bbox"]).float().to(gpu_device), solver,
                                        [{}, dict(overlap=True)])
    print(f"rtdetr r18: {n_ok} solved poses over the pipeline runs")
