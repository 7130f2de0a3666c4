"""CPU: the exhaustive four-point-subset solver's host side (ExhaustivePoseSolver, build_solver, the
argument checks of spe_pnp_exhaustive) and its numpy restatement (tests/pnp_exhaustive_ref.py, the
checker of the GPU tests) on hand-made cases."""
import ctypes
import itertools
from argparse import Namespace

import numpy as np
import pytest

import pnp_exhaustive_ref as X
import pnp_ref
from helpers import solver_stress_set
from spe import _lib
from spe.config import Camera, world_points
from spe.solver import EPnPCeresSolver, ExhaustivePoseSolver, build_solver

K = Camera.K
W = world_points()
ONES = np.ones((11, 2), np.float32)
STRESS_SEED = 0          # tests/test_gpu_pnp_exhaustive.py takes the same


def _case(seed, noise=0.0, nout=0, n=11):
    return X.synthetic_case(seed, noise, nout, n, K=K, world=W)


# ------------------------------------------------------------------------------------ host side
def test_build_solver_returns_the_exhaustive_solver():
    s = build_solver(Namespace(solver="exhaustive", topk=7, input_size=320))
    assert type(s) is ExhaustivePoseSolver
    assert (s.topk, s.input_size, s.reprojectionError, s.mode) == (7, 320, 20.0, 5) and _lib.SPE_PNP_EXHAUSTIVE == 5
    d = build_solver(Namespace(solver="exhaustive"))
    assert (d.topk, d.input_size) == (10, 256)
    # the threshold rule is EPnPCeresSolver's get_repro_th
    c = EPnPCeresSolver(256)
    for area in (10.0, 100.0, 300.0, 511.9, 512.0, 5000.0):
        assert d.repro_th(area) == c.repro_th(area) == pnp_ref.repro_th(area, 256)
    assert d.get_repro_th(100.0) == d.reprojectionError == 3.0


@pytest.mark.parametrize("topk", [0, 65, -1, 400])
def test_topk_out_of_range_is_refused_by_python(topk):
    with pytest.raises(ValueError, match="topk"):
        ExhaustivePoseSolver(topk=topk)
    with pytest.raises(ValueError, match="topk"):
        build_solver(Namespace(solver="exhaustive", topk=topk))


def _c_call(topk, C=12, fn="spe_pnp_exhaustive"):
    L = _lib.lib()
    d = ctypes.c_void_p(16)           # never dereferenced: the argument checks come first
    return getattr(L, fn)(None, d, d, None, 1, 11, C, d, d, 20.0, topk, d, d, None, None, None, None, None, None,
                          None, None)


@pytest.mark.parametrize("topk", [0, 65])
def test_topk_out_of_range_is_refused_by_c(topk):
    assert _c_call(topk) == -1
    assert b"topk" in _lib.lib().spe_last_error()


def test_too_many_classes_and_mode_5_through_the_batch_entry_are_refused():
    L = _lib.lib()
    assert _c_call(10, C=18) == -1                       # C - 1 > 16
    d = ctypes.c_void_p(16)
    rc = L.spe_pnp_batch(None, d, d, None, 1, 11, 12, d, d, 5, 20.0, 100, 0.99, d, d, None, None, None, None, None,
                         None)
    assert rc == -1 and b"bad solver mode" in L.spe_last_error()
    assert L.spe_abi_version() == 9


# ------------------------------------------------------------------------------------ the restatement
def test_subset_order_is_itertools_combinations():
    for n in (4, 5, 11, 16):
        S = X.subsets(n)
        assert S == list(itertools.combinations(range(n), 4)) == sorted(S)
    assert len(X.subsets(11)) == 330 and len(X.subsets(16)) == 1820


def test_clean_image_picks_a_zero_error_subset_and_keeps_the_threshold():
    wld, img, r, t = _case(1)
    o = X.exhaustive_pnp(wld, img, ONES, K, 20.0, 10)
    assert o["status"] == pnp_ref.ST_OK
    assert o["errors"][o["cand_index"]] < 1e-6            # px^2: float32 rounding of the projections only
    assert o["repro_final"] == np.float32(20.0)
    assert o["inlier_mask"] == (1 << 11) - 1
    assert all(tr[2] == 11 for tr in o["trace"]) and len(o["trace"]) == 10
    assert np.abs(o["tvec"] - t).max() < 1e-5 and np.abs(o["rvec"] - r).max() < 1e-5


def test_three_gross_outliers_among_eleven_points():
    wld, img, r, t = _case(1, nout=3)
    o = X.exhaustive_pnp(wld, img, ONES, K, 20.0, 10)
    assert o["status"] == pnp_ref.ST_OK
    assert o["inlier_mask"] == 0b11111111000               # the 8 clean points
    assert not set(X.subsets(11)[o["cand_index"]]) & {0, 1, 2}
    assert np.abs(o["tvec"] - t).max() < 1e-5 and np.abs(o["rvec"] - r).max() < 1e-5


def test_threshold_grows_by_5_per_failing_candidate():
    wld, img, _, _ = _case(3, noise=6.0)
    o = X.exhaustive_pnp(wld, img, ONES, K, 1.5, 10)
    ths = [tr[1] for tr in o["trace"]]
    fails = [tr[2] < 4 for tr in o["trace"]]
    assert len(o["trace"]) == 10 and fails[0] is False and any(fails)     # one pass; a later candidate fails
    s = 0
    for th, f in zip(ths, fails):                          # th0 + 5 per failure so far, carried over
        assert th == 1.5 + 5 * s
        s += f
    assert o["repro_final"] == np.float32(1.5 + 5 * s) and s >= 1
    # a first candidate below 4 inliers: the threshold it failed with is not the one the rest see
    wld, img, _, _ = _case(0, noise=6.0)
    o = X.exhaustive_pnp(wld, img, ONES, K, 1.5, 10)
    assert o["trace"][0][1:3] == (1.5, 3) and o["trace"][1][1] == 6.5 and o["status"] == pnp_ref.ST_OK
    # topk = 1: the walk repeats with the grown threshold until the one candidate has 4 inliers
    o1 = X.exhaustive_pnp(wld, img, ONES, K, 1.5, 1)
    assert [tr[1] for tr in o1["trace"]] == [1.5, 6.5] and o1["repro_final"] == np.float32(6.5)
    assert o1["cand_index"] == o1["candidates"][0]


def test_revert_if_worse_keeps_the_unrefined_pose():
    """A hypothesis already at the optimum of the summed error over all points: the LM on its inliers
    (a different cost) moves away from it, the refined sum is larger, the EPnP pose is kept and wins."""
    wld, img, _, _ = _case(2, noise=1.0)
    o = X.exhaustive_pnp(wld, img, ONES, K, 20.0, 10)
    reverted = [tr[0] for tr in o["trace"] if tr[3]]
    assert reverted == [o["cand_index"]]
    poses, _ = X.hypotheses(wld, img, K)
    np.testing.assert_array_equal(o["rvec"], poses[o["cand_index"], :3])
    np.testing.assert_array_equal(o["tvec"], poses[o["cand_index"], 3:])


def test_n_4_3_and_0():
    probs = np.full((11, 12), 0.01, np.float32)
    probs[:, 11] = 0.89                                    # every query: no object
    pts = np.zeros((11, 2), np.float32)
    wld, img, r, t = _case(4)
    r0 = X.solve_one(pts, probs, None, K, W, 20.0, 10)
    assert (r0["status"], r0["n_corr"], r0["cand_index"]) == (pnp_ref.ST_NO_FG, 0, -1)
    for n, st in ((3, pnp_ref.ST_CV_ERROR), (4, pnp_ref.ST_OK)):
        p = probs.copy()
        p[np.arange(n), np.arange(n)] = 0.95
        pts[:n] = img[:n]
        o = X.solve_one(pts, p, None, K, W, 20.0, 10)
        assert (o["status"], o["n_corr"]) == (st, n)
        assert o["repro_final"] == np.float32(20.0)
        if n == 4:
            assert o["cand_index"] == 0 and len(o["errors"]) == 1 and o["inlier_mask"] == 0b1111
            assert np.abs(o["tvec"] - t).max() < 1e-4
        else:
            assert o["cand_index"] == -1 and not o["quat"].any() and not o["tvec"].any()


def test_a_non_finite_subset_is_never_selected():
    wld, img, _, _ = _case(1)
    best = X.exhaustive_pnp(wld, img, ONES, K, 20.0, 10)
    h = best["candidates"][0]
    o = X.exhaustive_pnp(wld, img, ONES, K, 20.0, 330, force_nonfinite=(h,))
    assert np.isinf(o["errors"][h]) and h not in o["candidates"] and len(o["candidates"]) == 329
    assert o["status"] == pnp_ref.ST_OK and o["cand_index"] != h
    # nothing finite: no pose, the reference would not return
    wld4, img4 = wld[:4], img[:4]
    o = X.exhaustive_pnp(wld4, img4, ONES[:4], K, 20.0, 10, force_nonfinite=(0,))
    assert (o["status"], o["cand_index"]) == (pnp_ref.ST_UNPINNED, -1) and not o["tvec"].any()


def test_stable_topk_breaks_ties_by_subset_index():
    e = np.array([3, 1, 2, 1, np.inf, 1, 0.5], np.float32)
    assert X.stable_topk(e, 3) == [6, 1, 3]
    assert X.stable_topk(e, 64) == [6, 1, 3, 5, 2, 0]      # capped at the finite records


def test_pass_bound_of_the_kernel_never_skips_a_pass_that_can_succeed():
    """The refinement kernel skips the passes below first_pass_bound and walks at most 5 from there:
    the literal walk's first successful pass lies in [bound, bound + 4]."""
    rng = np.random.default_rng(0)
    for _ in range(4000):
        k = int(rng.integers(1, 65))
        th0 = float(rng.choice([1.5, 3.0, 20.0, 7.25]))
        e4 = rng.uniform(0, rng.choice([5, 50, 3000, 40000]), k).astype(np.float32)
        s = 0
        while not float(e4[s % k]) < th0 + 5.0 * s:
            s += 1
        b = X.first_pass_bound(e4, th0, k)
        assert b <= s // k <= b + 4, (k, th0, e4)


def test_stress_seed_has_few_near_ties():
    """The GPU parity test may leave out an image whose K-th and (K+1)-th errors nearly tie, 2 % of the
    batch at the most: the seed it uses stays under that in the restatement alone."""
    pts, probs, _, _, sig = solver_stress_set(96, STRESS_SEED)
    o = X.solve_batch(pts, probs, sig, K, W, 20.0, 10)
    assert (o["status"] == pnp_ref.ST_OK).sum() >= 0.8 * 96
    for topk in (1, 10, 64):
        n = sum(X.near_tie(e, topk) for e in o["errors"] if len(e))
        assert n <= 0.02 * 96, (topk, n)
