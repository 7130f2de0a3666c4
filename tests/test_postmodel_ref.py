"""CPU pins of the references that tests/test_gpu_postmodel_edges.py compares the device against.

* oracle/ensemble_ref.pairwise_sum == np.add.reduce, bit for bit, at every pool size up to the
  contract's M * Q = 256 (above 128 values numpy splits the sum; the restatement and the kernel once
  stopped at one block and were a last bit off from n = 129 on);
* oracle/ensemble_ref.mean_and_filter / fuse_batch == the numpy-direct fusion of
  tests/postmodel_ref.py, bit for bit and NaN for NaN, at those sizes and on every device case;
* oracle/criterion_ref.lsap == scipy's linear_sum_assignment on matrices with repeated rows and
  columns at the device cases' shapes, and the loss restatement at num_classes != 12 against torch's
  own weighted cross entropy;
* the solver sets of the device test: the share of images that solve, and the 16-label image.
"""
import numpy as np
import pytest

import criterion_ref as cr
import ensemble_ref as er
import postmodel_ref as pr


@pytest.mark.parametrize("n", pr.POOL_SIZES + (130, 135, 250))
def test_pairwise_sum_is_numpys(n):
    rng = np.random.default_rng(n)
    for k in range(100):
        a = rng.exponential(3.0, n) if k % 2 else rng.normal(0, 1e3, n)
        assert er.pairwise_sum(a) == np.add.reduce(a), (n, k)
        mu = er.pairwise_sum(a) / n
        assert np.sqrt(er.pairwise_sum((a - mu) ** 2) / n) == np.std(a), (n, k)


@pytest.mark.parametrize("n", pr.POOL_SIZES)
def test_mean_and_filter_is_numpy_direct(n):
    rng = np.random.default_rng(1000 + n)
    dropped = 0
    for _ in range(40):
        p = pr.pool_points(rng, n, outliers=0.1)
        ref = pr.mean_and_filter_numpy(p)
        got = er.mean_and_filter(p)
        assert got.dtype == np.float32 and np.array_equal(got, ref, equal_nan=True), (n, got, ref)
        dropped += not np.array_equal(ref, p.mean(0), equal_nan=True)
    if n >= 7:
        assert dropped > 0                                   # the filter did drop points in some pools


def test_fusion_restatement_is_numpy_direct_on_the_device_cases():
    for name, (pts, prb) in pr.ensemble_cases().items():
        C = prb.shape[-1]
        rp, rr = pr.fuse_batch_numpy(pts, prb)
        op, orr = er.fuse_batch(pts, prb, num_classes=C)
        assert np.array_equal(orr, rr), name
        assert np.array_equal(op, rp, equal_nan=True), name
    # what the cases are there for
    cases = pr.ensemble_cases()
    rp, rr = pr.fuse_batch_numpy(*cases["c17_all_labels"])
    assert (rr[:, :, 16] == 0).all()                         # 16 labels seen in every image
    assert list(rr[0].argmax(1)) == [9, 3, 15, 0, 12, 7, 1, 14, 5, 10, 2, 8, 13, 4, 11, 6]
    rp, rr = pr.fuse_batch_numpy(*cases["coincide_and_no_foreground"])
    assert np.isnan(rp[0, 0]).all() and np.isfinite(rp[0, 1]).all() and (rr[1, :, 11] == 1).all()
    rp, rr = pr.fuse_batch_numpy(*cases["argmax_ties"])
    assert rr[0, 0, 0] == 1 and (rr[:, :, 3].sum(1) == 1).all()
    for name, n in (("one_label_256", 256), ("one_label_129", 129), ("one_label_255", 255)):
        pts, prb = cases[name]
        assert ((prb.argmax(-1) != 11).sum((0, 2)) == n).all()


@pytest.mark.parametrize("shape", [(64, 32), (64, 1), (32, 32), (1, 1), (33, 32), (40, 11), (11, 11), (11, 40), (12, 5)])
def test_lsap_ties_match_scipy(shape):
    from scipy.optimize import linear_sum_assignment
    for c in pr.tie_matrices(shape, seed=shape[0] * 100 + shape[1]):
        r0, c0 = linear_sum_assignment(c)
        r1, c1 = cr.lsap(c)
        assert np.array_equal(r0, r1) and np.array_equal(c0, c1), c


@pytest.mark.parametrize("kind", ["queries", "targets", "labels"])
def test_criterion_tie_cases_tie_and_match_scipy(kind):
    """The tie cases do hold exactly equal costs, and the restated assignment on them is scipy's."""
    from scipy.optimize import linear_sum_assignment
    for Q, T in ((8, 8), (12, 5)):
        logits, points, labels, tpts = pr.criterion_tie_case(kind, Q, T)
        _, m0 = cr.criterion([(logits[0], points[0])], labels, tpts)
        _, m1 = cr.criterion([(logits[0], points[0])], labels, tpts, solver=linear_sum_assignment)
        assert np.array_equal(m0, m1)
        cp = np.abs(points[0, 0][:, None] - tpts[0][None]).sum(-1)
        if kind == "queries":
            assert np.array_equal(cp[0], cp[1])
        elif kind == "targets":
            assert np.array_equal(cp[:, 0], cp[:, 1])
        else:
            assert len(set(labels[0])) <= 2


@pytest.mark.parametrize("C", [2, 12, 32])
def test_criterion_restatement_at_other_class_counts(C):
    """loss_ce with no-object = C - 1 (the reference's 11 at C = 12) against torch's weighted cross entropy, and
    out-of-range labels clamped to C - 1 == the run on the clamped labels."""
    import torch
    import torch.nn.functional as F
    logits, points, labels, tpts = pr.criterion_case(C, 1, 5, 9, 4, C)
    losses, match = cr.criterion([(logits[0], points[0])], labels, tpts)
    tc = np.full((5, 9), C - 1, np.int64)
    for b in range(5):
        tc[b, match[0, b]] = labels[b]
    w = torch.ones(C, dtype=torch.float64)
    w[-1] = 0.1
    ce = F.cross_entropy(torch.from_numpy(logits[0]).double().transpose(1, 2), torch.from_numpy(tc), w)
    assert abs(losses["loss_ce"] - float(ce)) <= 1e-9
    assert abs(losses["cardinality_error"] - np.abs((logits[0].argmax(-1) != C - 1).sum(1) - 4).mean()) == 0


SOLVER_SHAPES = [(64, 12), (40, 12), (30, 17), (64, 17), (4, 12), (1, 12)]


@pytest.mark.parametrize("Q,C", SOLVER_SHAPES)
def test_solver_sets_mostly_solve(Q, C):
    """The oracle solves at least half of every device case with Q >= 11 in every mode (so the device
    test's pose comparison is not vacuous), and a C = 17 set holds an image with all 16 labels."""
    import pnp_ref
    from spe.config import Camera
    pts, probs, q, t, sig, th = pr.solver_set(48, Q, C, seed=Q * 100 + C)
    for mode in range(5):
        o = pnp_ref.pnp_batch(pts, probs, Camera.K, pr.world_for(C), mode=mode, repro=25.0 if mode == 2 else 20.0,
                              sigmas=sig if mode in (2, 4) else None, repro_per_image=th if mode == 4 else None)
        ok = (o["status"] == 0) | (o["status"] == 3)
        if Q >= 11:
            assert ok.sum() >= 24, (mode, int(ok.sum()))
        if C == 17:
            assert (o["n_corr"] == 16).any()
        assert o["n_corr"].max() <= min(Q, C - 1)
