"""CPU: the pose covariance's definition (include/spe.h spe_pose_covariance) as restated in
tests/pose_covariance_ref.py -- its Jacobian against central differences, the covariance against a
Monte-Carlo re-solve, the status rules -- and the C ABI entry."""
import numpy as np

import pose_covariance_ref as pc

K, W, C = pc.K, pc.W, pc.C


def test_jacobian_matches_central_differences():
    """Step h = 1e-6 on each of the six perturbation coordinates.  The differencing error has two
    parts.  Truncation: h^2 / 6 times the third derivative, which for a projection at depth z of a point
    of lever arm |RX| <= 1 m is of the order of the first derivative itself (every further derivative
    brings a factor <= max(1, |RX|) / z < 1), so <= ~1e-12 relative.  Rounding: the two projections are
    pixels of size |u| <= ~2e3 (principal point 960 px + offset) carrying eps |u| each, so the quotient
    carries <= eps |u| / h = 2.2e-16 * 2e3 / 1e-6 = 4.4e-7 px per unit, against max |J| = fx / z >= 250
    px per unit at z <= 12 m: <= 2e-9 relative.  The bound 1e-7 of max |J| leaves a factor 50."""
    h = 1e-6
    worst = 0.0
    for seed in range(6):
        R, t = pc.pose(seed, z=4.0 + 1.6 * seed)
        for X in W:
            J = pc.jacobian(R, t, X, K)
            num = np.zeros((2, 6))
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                up = pc.project(*pc.perturbed(R, t, d), X[None], K)[0]
                dn = pc.project(*pc.perturbed(R, t, -d), X[None], K)[0]
                num[:, k] = (up - dn) / (2 * h)
            worst = max(worst, np.abs(J - num).max() / np.abs(J).max())
    print("jacobian: worst relative difference", worst)
    assert worst <= 1e-7


def test_covariance_predicts_monte_carlo_spread():
    """N = 4000 draws of Gaussian pixel noise with the given sigmas (anisotropic, 0.1 .. 0.5 px) on the 11
    landmarks at 10 m, each re-solved by two Gauss-Newton steps from the true pose (the first is the
    linear solution, the second removes its second-order remainder).  Each sample variance is within
    6 sqrt(2 / (N - 1)) relative of the predicted diagonal: six standard errors of a variance estimate."""
    N = 4000
    rng = np.random.default_rng(2024)
    R, t = pc.pose(11, z=10.0)
    sig = rng.uniform(0.1, 0.5, (C - 1, 2)).astype(np.float32)
    o = pc.pose_covariance(**pc.one_image(R, t, sig), sigma_floor=1e-3)
    assert o["cov_status"][0] == 0
    pred = np.diag(o["cov"][0])
    uv0 = pc.project(R, t, W, K)
    sg = sig.astype(np.float64)
    d = np.stack([pc.gauss_newton(R, t, W, uv0 + rng.normal(size=uv0.shape) * sg, sg, K, steps=2) for _ in range(N)])
    var = d.var(axis=0, ddof=1)
    gate = 6 * np.sqrt(2.0 / (N - 1))
    rel = np.abs(var / pred - 1)
    print("monte carlo: relative deviation of the six variances", rel, "gate", gate)
    assert rel.max() <= gate
    # the off-diagonal structure too, loosely: the sample correlation matrix against the predicted one
    s = np.sqrt(pred)
    assert np.abs(np.cov(d.T) / np.outer(s, s) - o["cov"][0] / np.outer(s, s)).max() <= 2 * gate
    # and the derived outputs are what they say
    assert np.isclose(o["sigma_rot"][0], np.sqrt(pred[:3].sum()))
    assert np.allclose(o["sigma_t"][0], np.sqrt(pred[3:]))
    assert np.isclose(o["pred_score"][0], np.sqrt(pred[:3].sum()) + np.sqrt(pred[3:].sum()) / np.linalg.norm(t))


def test_status_rules():
    for name, (inp, want) in pc.status_cases().items():
        o = pc.pose_covariance(**inp)
        assert o["cov_status"][0] == want, (name, o["cov_status"][0], o["min_pivot"][0])
        if want:
            assert not o["cov"].any() and not o["sigma_t"].any() and o["sigma_rot"][0] == 0 and o["pred_score"][0] == 0
        else:
            assert np.all(np.linalg.eigvalsh(o["cov"][0]) > 0)
    # precedence: no pose before the inlier count before the sigma
    inp, _ = pc.status_cases()["nan_sigma"]
    inp["inlier_mask"][:] = 0b11
    assert pc.pose_covariance(**inp)["cov_status"][0] == 2
    inp["status"][:] = 1
    assert pc.pose_covariance(**inp)["cov_status"][0] == 1


def test_sigma_scale_and_floor():
    R, t = pc.pose(9, z=9.0)
    sig = np.random.default_rng(1).uniform(0.001, 0.004, (C - 1, 2)).astype(np.float32)   # crop-normalised
    scale = np.array([[256.0, 512.0]], np.float32)          # powers of two: the float32 product is exact
    a = pc.pose_covariance(**pc.one_image(R, t, sig), sigma_scale=scale)
    b = pc.pose_covariance(**pc.one_image(R, t, sig * scale[0]))
    assert a["cov_status"][0] == 0
    np.testing.assert_array_equal(a["cov"], b["cov"])
    # the floor takes over below it: every sigma under the floor gives the floor's covariance
    lo = pc.pose_covariance(**pc.one_image(R, t, np.full((C - 1, 2), 1e-6, np.float32)), sigma_floor=0.25)
    fl = pc.pose_covariance(**pc.one_image(R, t, np.full((C - 1, 2), 0.25, np.float32)), sigma_floor=0.25)
    np.testing.assert_array_equal(lo["cov"], fl["cov"])


def test_abi_exports_pose_covariance():
    import os
    import re
    from conftest import REPO
    from spe import _lib
    L = _lib.lib()
    assert "spe_pose_covariance" in _lib.EXPORTS
    assert hasattr(L, "spe_pose_covariance")
    assert len(L.spe_pose_covariance.argtypes) == 20
    assert re.search(r"^int spe_pose_covariance\(", open(os.path.join(REPO, "include", "spe.h")).read(), re.M)
    assert L.spe_abi_version() == _lib.ABI_VERSION == 9
