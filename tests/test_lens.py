"""CPU: the lens model's definition (include/spe.h spe_undistort_points) as restated in tests/lens_ref.py
-- round trip, the Jacobian against central differences -- and what needs no device of the C ABI and
the Python layer: the exports, the argument refusals, LensModel, build_solver."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

import lens_ref as lr

K, DIST = lr.K, lr.DIST


def test_round_trip_on_the_frame_grid():
    """distort then undistort over the 117 x 81 grid (frame + 200 px): the fixed-point iteration
    contracts by about |k1| r2 ~ 0.05 per round at the corners, measured 2.9e-7 px after 5 rounds and
    9e-13 px after 12 (the fp64 floor at |u| ~ 2e3 px)."""
    g = lr.frame_grid()
    d = lr.distort(g, K, DIST)
    shift = np.abs(d - g).max()
    print("largest shift per axis", shift, "px")
    assert 30.0 < shift < 31.0
    for iters, bound in ((5, 1e-6), (12, 1e-11)):
        u, st, _, _ = lr.undistort(d, K, DIST, iters)
        err = np.abs(u - g).max()
        print("round trip, iters", iters, err, "px")
        assert not st.any()
        assert err <= bound


def test_jacobian_matches_central_differences():
    """h = 1e-3 px: truncation h^2 / 6 * D''' ~ 1e-6 * 1e-6 (the map's third derivative in pixels is
    ~ k1 / fx^2), rounding eps * |u| / h = 2.2e-16 * 2e3 / 1e-3 = 4e-10, against entries of order 1."""
    g = lr.frame_grid()
    fx, fy, cx, cy = lr._k(K)
    D = np.array(lr.jacobian((g[:, 0] - cx) / fx, (g[:, 1] - cy) / fy, K, DIST))      # D11, D12, D21, D22
    h = 1e-3
    worst = 0.0
    for k in range(2):
        e = np.zeros(2)
        e[k] = h
        num = (lr.distort(g + e, K, DIST) - lr.distort(g - e, K, DIST)) / (2 * h)       # column k of D
        an = np.stack((D[k], D[2 + k]), 1)
        worst = max(worst, np.abs(num - an).max() / np.abs(an).max())
    print("jacobian: worst relative difference", worst)
    assert worst <= 1e-6
    stretch = np.abs(D - np.array([1.0, 0, 0, 1.0])[:, None])
    inside = (g[:, 0] >= 0) & (g[:, 0] <= 1920) & (g[:, 1] >= 0) & (g[:, 1] <= 1200)
    print("max |D - I| over the frame", stretch[:, inside].max(), "with the margin", stretch.max())


def test_sigma_rule_is_the_diagonal_of_the_mapped_covariance():
    rng = np.random.default_rng(5)
    p = lr.random_points(rng, (2, 9))
    s = rng.uniform(0.5, 3.0, (2, 9, 2)).astype(np.float32)
    o = lr.undistort_points(p, s)
    _, _, x, y = lr.undistort(p, K, DIST, 5)
    d11, d12, d21, d22 = lr.jacobian(x, y, K, DIST)
    for b in range(2):
        for q in range(9):
            A = np.linalg.inv(np.array([[d11[b, q], d12[b, q]], [d21[b, q], d22[b, q]]]))
            cov = A @ np.diag(s[b, q].astype(np.float64) ** 2) @ A.T
            np.testing.assert_allclose(o["sigmas64"][b, q], np.sqrt(np.diag(cov)), rtol=1e-12)
    # a crop-normalised sigma with its scale is the pixel sigma's result, normalised again
    sc = np.array([[256.0, 512.0], [128.0, 64.0]], np.float32)         # powers of two: exact products
    n = lr.undistort_points(p, s / sc[:, None, :], sc)
    np.testing.assert_allclose(n["sigmas64"] * sc[:, None, :], o["sigmas64"], rtol=1e-14)


def test_zero_distortion_is_a_copy_and_bad_icd_returns_the_input():
    rng = np.random.default_rng(6)
    p = lr.random_points(rng, (1, 5))
    s = rng.uniform(0.5, 3.0, (1, 5, 2)).astype(np.float32)
    o = lr.undistort_points(p, s, dist=np.zeros(5))
    assert o["points"].tobytes() == p.tobytes() and o["sigmas"].tobytes() == s.tobytes() and not o["status"].any()
    # k1 = -5 at r2 = 0.25: 1 + k1 r2 = -0.25, icd < 0 in round 1
    fx, fy, cx, cy = lr._k(K)
    p[0, 2] = (cx + 0.5 * fx, cy)
    p[0, 0] = (cx + 0.1 * fx, cy)                 # r2 = 0.01: in the domain
    b = lr.undistort_points(p, s, dist=np.array([-5.0, 0, 0, 0, 0]))
    assert b["status"][0, 2] == 1 and b["status"][0, 0] == 0
    assert b["points"][0, 2].tobytes() == p[0, 2].tobytes() and b["sigmas"][0, 2].tobytes() == s[0, 2].tobytes()
    assert b["points"][0, 0, 0] != p[0, 0, 0]


def test_abi_exports_the_lens_entries():
    from conftest import REPO
    from spe import _lib
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "spe.h")).read()
    for name, nargs in (("spe_undistort_points", 12), ("spe_distort_points", 7)):
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs
        assert re.search(r"^int %s\(" % name, header, re.M)
    assert L.spe_abi_version() == _lib.ABI_VERSION == 9


def test_argument_refusals_need_no_device():
    """Every refusal comes before any launch, so host buffers stand in for the device arrays."""
    from spe import _lib
    L = _lib.lib()
    pts = (ctypes.c_float * 8)()
    sig = (ctypes.c_float * 8)()
    out = (ctypes.c_float * 8)()
    sout = (ctypes.c_float * 8)()
    Kb = (ctypes.c_double * 9)(*K.ravel())
    db = (ctypes.c_double * 5)(*DIST)
    a = ctypes.addressof

    def call(batch=1, q=4, iters=5, sigmas=a(sig), sigmas_ideal=a(sout)):
        return L.spe_undistort_points(None, a(pts), sigmas, None, batch, q, a(Kb), a(db), iters, a(out),
                                      sigmas_ideal, None)
    E_ARG = -1
    assert call(iters=0) == E_ARG
    assert call(iters=65) == E_ARG
    assert call(batch=0) == E_ARG
    assert call(q=0) == E_ARG
    assert call(sigmas=None) == E_ARG                      # sigmas_ideal without sigmas
    assert b"sigmas_ideal" in L.spe_last_error()
    assert L.spe_distort_points(None, a(pts), 0, 4, a(Kb), a(db), a(out)) == E_ARG
    assert L.spe_distort_points(None, a(pts) + 4, 1, 3, a(Kb), a(db), a(out)) == E_ARG     # not 8-byte aligned


def test_lens_model_takes_four_or_five_coefficients():
    from spe.config import Camera, LensModel
    m = LensModel()
    assert not m.dist.any() and m.dist.shape == (5,) and m.iters == 5 and (m.K == Camera.K).all()
    assert LensModel(dist=DIST).dist.tolist() == DIST.tolist()
    four = LensModel(dist=DIST[:4])
    assert four.dist[:4].tolist() == DIST[:4].tolist() and four.dist[4] == 0
    for n in (3, 6):
        with pytest.raises(ValueError):
            LensModel(dist=np.zeros(n))
    for iters in (0, 65):
        with pytest.raises(ValueError):
            LensModel(dist=DIST, iters=iters)
    with pytest.raises(Exception):
        m.iters = 7                                        # frozen
    with pytest.raises(ValueError):
        m.dist[0] = 1.0                                    # and its arrays are read-only
    assert LensModel.from_args(argparse.Namespace(dist=list(DIST))).dist.tolist() == DIST.tolist()
    assert not LensModel.from_args(argparse.Namespace()).dist.any()


def test_build_solver_without_dist_has_no_lens():
    from spe.solver import build_solver
    for name in ("ransac_p3p_lm", "epnp_ransac_sigma", "epnp", "epnp_lm", "epnp_ceres", "exhaustive", "ensemble_sigma"):
        assert build_solver(argparse.Namespace(solver=name)).lens is None
        s = build_solver(argparse.Namespace(solver=name, dist=list(DIST[:4])))
        assert s.lens.dist.tolist() == list(DIST[:4]) + [0.0]
    assert build_solver().lens is None


def test_project_with_dist_is_the_reference_distort():
    from spe.config import project, world_points
    q, t = np.array([0.9, 0.1, -0.3, 0.2]), np.array([0.3, -0.2, 6.0])
    W = world_points()
    ideal = project(W, q, t)
    np.testing.assert_allclose(project(W, q, t, dist=DIST), lr.distort(ideal, K, DIST), rtol=0, atol=1e-9)
    np.testing.assert_allclose(project(W, q, t, dist=np.zeros(5)), ideal, rtol=0, atol=1e-9)


def test_sigma_ensemble_refuses_a_second_lens_on_its_backend():
    from spe.config import LensModel
    from spe.solver import SigmaEnsemblePoseSolver, SimplePoseSolverSigma
    a, b = LensModel(dist=DIST), LensModel(dist=DIST[:4])
    backend = SimplePoseSolverSigma()
    ens = SigmaEnsemblePoseSolver(backend, lens=a)
    assert ens.lens is a and backend.lens is a and (backend.K == a.K).all()
    assert SigmaEnsemblePoseSolver(backend, lens=a).lens is a          # the same lens again is fine
    with pytest.raises(ValueError):
        SigmaEnsemblePoseSolver(backend, lens=b)
    assert SigmaEnsemblePoseSolver(SimplePoseSolverSigma()).lens is None
