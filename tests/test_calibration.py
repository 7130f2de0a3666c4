"""CPU: the calibration records' definition (include/spe.h spe_calibration_records) as restated in
tests/calibration_ref.py -- the rotation error against the SPEED score's angle, the ground-truth rotation
against the solver's quaternion conversion, the summary's sparsification / AUSE / Spearman / threshold on
hand-sized arrays (the reference and spe.calibration's own code, on CPU tensors), and the statistical
consistency of the definition itself -- plus the C ABI entry."""
import math

import numpy as np
import pytest

import calibration_ref as cr
import pnp_ref
import pose_covariance_ref as pc

EPS = np.finfo(np.float64).eps


def test_rotation_error_norm_is_the_speed_score_angle():
    """|dw| of the reference against speed_score's s_q = 2 acos(|q_pr . q_gt|) on random pose pairs whose
    relative angle is 1e-6 .. 3 rad.  Both sides start from the same two unit quaternions (entries rounded to
    eps).  s_q: the dot product c = cos(a / 2) carries <= 4 eps (four products, three sums, two roundings of
    unit inputs), and d acos / dc = -1 / sin(a / 2), so s_q carries <= 2 * 4 eps / sin(a / 2) plus acos's own
    rounding, eps * s_q.  |dw|: R_pr and R_gt carry <= ~8 eps per entry, their product <= ~30 eps, the
    quaternion's vector part read off it <= ~20 eps absolute, so |dw| = 2 atan2(|v|, w) carries <= ~40 eps absolute
    whatever the angle.  The bound is their sum with a factor 2: 2 (8 eps / sin(a / 2) + 40 eps + eps a).  At
    a = 1e-6 that is 7e-9 rad: the arccos side dominates, which is why the definition avoids it."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for ang in (1e-6, 1e-5, 1e-3, 0.1, 1.0, 3.0) * 8:
        q_gt = rng.normal(size=4)
        q_gt /= np.linalg.norm(q_gt)
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        R_gt = pc.quat_to_R(q_gt)
        R_pr = pc.rodrigues(ax * ang) @ R_gt
        d = cr.pose_error(R_pr, np.zeros(3), q_gt, np.zeros(3))
        # the predicted pose's quaternion, for the score: q_rel (x) q_gt in fp64
        w, v = math.cos(ang / 2), ax * math.sin(ang / 2)
        q_pr = np.concatenate([[w * q_gt[0] - v @ q_gt[1:]], w * q_gt[1:] + q_gt[0] * v + np.cross(v, q_gt[1:])])
        _, s_q = pnp_ref.speed_score(q_pr, np.ones(3), q_gt, np.ones(3))
        bound = 2 * (8 * EPS / math.sin(ang / 2) + 40 * EPS + EPS * ang)
        err = abs(np.linalg.norm(d[:3]) - s_q)
        worst = max(worst, err / bound)
        assert err <= bound, (ang, err, bound)
        # and the error itself is the rotation put in, to the matrix side's 40 eps
        assert np.abs(d[:3] - ax * ang).max() <= 40 * EPS + 2 * EPS * ang, (ang, d[:3] - ax * ang)
    print("angle: largest error / bound", worst)


def test_ground_truth_rotation_inverts_the_solver_quaternion():
    """R -> q = blender_quat(R) (the oracle's restatement of the solver's conversion, float32) -> R_gt(q)
    returns R to the conversion's float32 rounding, and a pose that emits q_gt has zero rotation error against it.
    The rounding: the conversion forms w = sqrt(tr), tr = (1 + trace) / 4 from float32 entries, an absolute error
    of <= 2^-24 in tr and so <= 2^-24 / (2 w) in w; its first branch runs down to tr = 1e-4, w = 0.01, where that
    is 3e-6 (the other branches divide by a pivot >= 1, and the final normalisation leaves the vector part's error
    second order).  R's entries are 2 (products of two components): <= 4 dw = 4 * 2^-24 / 0.02, plus 8 * 2^-24 for
    the other float32 roundings."""
    bound = 4 * 2.0 ** -24 / 0.02 + 8 * 2.0 ** -24
    rng = np.random.default_rng(3)
    for _ in range(50):
        R = pc.quat_to_R(rng.normal(size=4))
        q = pnp_ref.blender_quat(R).astype(np.float64)
        assert np.abs(pc.quat_to_R(q) - R).max() <= bound
        d = cr.pose_error(pc.quat_to_R(q), np.zeros(3), q, np.zeros(3))
        assert not d.any()


def test_chi2_constants_are_the_quantiles():
    from spe import calibration
    assert calibration.CHI2_6 == cr.CHI2_6 and calibration.CHI2_3 == cr.CHI2_3
    for dof, qs in ((6, cr.CHI2_6), (3, cr.CHI2_3)):
        for q, p in zip(qs, (0.5, 0.9, 0.99)):
            assert abs(cr.chi2_cdf(q, dof) - p) <= 4 * EPS
    for k, c in zip((1, 2, 3), cr.NORMAL_COVERAGE):
        assert abs(math.erf(k / math.sqrt(2)) - c) <= EPS


# ---------------------------------------------------------------- the summary on hand-sized arrays
def _product_summary(pred, score, cov_status=None):
    """spe.calibration.summarize_records on CPU tensors holding only what the sparsification reads."""
    import torch
    from spe.calibration import Calibration, summarize_records
    N = len(pred)
    r = dict(z=torch.zeros(N, 2, 2, dtype=torch.float64), kp_flags=torch.zeros(N, 2, dtype=torch.uint8),
             nees=torch.zeros(N, 3, dtype=torch.float64), calib_status=torch.full((N,), 3, dtype=torch.int32),
             score=torch.tensor(score, dtype=torch.float64), pred_score=torch.tensor(pred, dtype=torch.float64),
             cov_status=torch.tensor(cov_status if cov_status is not None else [0] * N, dtype=torch.int32))
    cal = Calibration()
    cal._host, s = summarize_records(r)
    return cal, s["sparsification"]


CASES = {
    # N = 4, removed = floor(k / 5): 0 for k < 5, 1 for k < 10, 2 for k < 15, 3 above.  pred has a tie between
    # images 1 and 2 (0.5): the order is 0, 1, 2, 3.  kept means by pred: all (1+4+2+3)/4 = 2.5; without image 0:
    # 3; without 0, 1: 2.5; image 3 alone: 3.  oracle order 1, 3, 2, 0: 2.5, 2, 1.5, 1.
    "ties": dict(pred=[0.75, 0.5, 0.5, 0.25], score=[1.0, 4.0, 2.0, 3.0],
                 by_pred=[2.5] * 5 + [3.0] * 5 + [2.5] * 5 + [3.0] * 5, oracle=[2.5] * 5 + [2.0] * 5 + [1.5] * 5 + [1.0] * 5,
                 # ranks by pred 0,1,2,3; by score: image 1 -> 0, 3 -> 1, 2 -> 2, 0 -> 3: d = 3,-1,0,-2, sum d^2 = 14
                 spearman=1 - 6 * 14 / (4 * 15)),
    # all predictions equal: the stable order is the image order 0, 1, 2, 3
    "all_equal": dict(pred=[0.5] * 4, score=[4.0, 3.0, 2.0, 1.0],
                      by_pred=[2.5] * 5 + [2.0] * 5 + [1.5] * 5 + [1.0] * 5, oracle=[2.5] * 5 + [2.0] * 5 + [1.5] * 5 + [1.0] * 5,
                      spearman=1.0),
    "one": dict(pred=[0.25], score=[2.0], by_pred=[2.0] * 20, oracle=[2.0] * 20, spearman=0.0),
}


def _ause(by_pred, oracle, mean):
    d = [a - b for a, b in zip(by_pred, oracle)]
    return sum(0.5 * (d[k] + d[k + 1]) / 20 for k in range(19)) / mean


@pytest.mark.parametrize("name", list(CASES))
def test_sparsification_on_hand_sized_arrays(name):
    c = CASES[name]
    ref = cr.sparsification(c["pred"], c["score"])
    _, got = _product_summary(c["pred"], c["score"])
    mean = sum(c["score"]) / len(c["score"])
    for s in (ref, got):
        assert s["count"] == len(c["pred"])
        assert s["by_pred"] == c["by_pred"] and s["oracle"] == c["oracle"] and s["random"] == [mean] * 20
        assert s["spearman"] == c["spearman"]
        assert s["ause"] == _ause(c["by_pred"], c["oracle"], mean)
        assert s["fractions"] == [k / 20 for k in range(20)]
    if name == "ties":
        # by hand: d = 0 (5 points), 1 (5), 1 (5), 2 (5): trapezoids 4*0 + .5 + 4*1 + 1 + 4*1 + 1.5 + 4*2 = 19, / 20 / 2.5
        # (the 19 terms are rounded quotients by 20: equal to a few roundings, not to the bit)
        assert abs(ref["ause"] - 19 / 20 / 2.5) <= 8 * EPS


def test_sparsification_skips_images_without_a_covariance():
    pred, score = [9.0, 0.75, 0.5, 0.5, 0.0, 0.25], [7.0, 1.0, 4.0, 2.0, 9.0, 3.0]
    cov_status = [1, 0, 0, 0, 4, 0]
    _, got = _product_summary(pred, score, cov_status)
    c = CASES["ties"]
    assert got["count"] == 4 and got["by_pred"] == c["by_pred"] and got["oracle"] == c["oracle"]
    assert got["spearman"] == c["spearman"]


def test_threshold_for_on_hand_sized_arrays():
    c = CASES["ties"]
    cal, _ = _product_summary(c["pred"], c["score"])
    # kept sets by threshold: 0.25 -> {3}: mean 3; 0.5 -> {1, 2, 3}: 3; 0.75 -> all: 2.5
    for risk, want in ((2.5, (0.75, 1.0)), (2.4, (None, 0.0)), (3.0, (0.75, 1.0)), (100.0, (0.75, 1.0))):
        assert cr.threshold_for(c["pred"], c["score"], risk) == want
        assert cal.threshold_for(risk) == want
    # a risk only the best-predicted images meet
    pred, score = [0.1, 0.2, 0.2, 0.9], [1.0, 2.0, 3.0, 10.0]
    cal, _ = _product_summary(pred, score)
    for risk, want in ((1.0, (0.1, 0.25)), (2.0, (0.2, 0.75)), (1.5, (0.1, 0.25)), (0.5, (None, 0.0)), (4.0, (0.9, 1.0))):
        assert cr.threshold_for(pred, score, risk) == want
        assert cal.threshold_for(risk) == want
    cal, _ = _product_summary([0.25], [2.0])
    assert cal.threshold_for(2.0) == (0.25, 1.0) and cal.threshold_for(1.0) == (None, 0.0)


# ---------------------------------------------------------------- the definition is statistically consistent
N_STAT = 512


def _experiment():
    """N_STAT images, keypoints = ground truth + 2 sigma noise, re-solved by three Gauss-Newton steps from the
    true pose with the 1 / sigma^2 weights (the path of test_pose_covariance's Monte-Carlo check), the
    covariance from the reference at the predicted (uncalibrated) sigmas."""
    pts, probs, sig, q_gt, t_gt, Rs = cr.experiment_inputs(N_STAT)
    N, Q, C = probs.shape
    labels = probs.argmax(2)
    rvec, tvec = np.zeros((N, 3)), np.zeros((N, 3))
    corr = np.full((N, 16), -1, np.int32)
    for b in range(N):
        X = pc.W[labels[b]]
        R1, t1 = cr.gauss_newton_pose(Rs[b], t_gt[b], X, pts[b].astype(np.float64), sig[b].astype(np.float64), pc.K)
        rvec[b], tvec[b] = cr.rvec_of(R1), t1
        corr[b, :Q] = labels[b]
    status = np.zeros(N, np.int32)
    mask = np.full(N, (1 << Q) - 1, np.uint32)
    cov = pc.pose_covariance(probs, sig, status, corr, mask, rvec, tvec, pc.K, pc.W)
    assert (cov["cov_status"] == 0).all()
    return dict(points=pts, probs=probs, sigmas=sig, status=status, corr_label=corr, inlier_mask=mask, rvec=rvec,
                tvec=tvec, q_gt=q_gt, t_gt=t_gt, cov=cov["cov"], cov_status=cov["cov_status"], K=pc.K, world=pc.W), cov


def test_definition_is_statistically_consistent():
    """The gates of the issue, N = 512 images of 11 landmarks (n = 11264 axis samples): the measured sigma_gain
    within 2 (1 +- 6 / sqrt(2 n)); with it applied the mean NEES within 6 +- 6 sqrt(12 / N) and the coverage at
    1, 2, 3 sigma within six binomial standard errors of the normal values.  Every image reaches status 0."""
    x, cov = _experiment()
    gate = cr.gates(N_STAT)
    score = np.zeros(N_STAT)
    rec = cr.calibration_records(**x)
    assert (rec["calib_status"] == 0).all() and (rec["kp_flags"] == 3).all()
    s1 = cr.summarize(rec, score, cov["pred_score"], cov["cov_status"])
    g = s1["sigma_gain"]
    print("sigma_gain", g, "gate", gate["sigma_gain"], "mean NEES at gain 1", s1["pose"]["mean_nees"])
    assert gate["sigma_gain"][0] <= g <= gate["sigma_gain"][1]
    # uncalibrated, the covariance is too small by g^2: the NEES shows it
    assert s1["pose"]["mean_nees"][0] > gate["mean_nees"][1]
    rec = cr.calibration_records(**x, sigma_gain=g)
    assert (rec["calib_status"] == 0).all()
    s2 = cr.summarize(rec, score, cov["pred_score"] * g, cov["cov_status"], sigma_gain=g)
    print("calibrated: mean NEES", s2["pose"]["mean_nees"], "gate", gate["mean_nees"], "coverage",
          s2["keypoints"]["inliers"]["coverage"], "gates", gate["coverage"], "shares", s2["pose"]["below_chi2"])
    assert gate["mean_nees"][0] <= s2["pose"]["mean_nees"][0] <= gate["mean_nees"][1]
    for c, (lo, hi) in zip(s2["keypoints"]["inliers"]["coverage"], gate["coverage"]):
        assert lo <= c <= hi
    assert abs(s2["sigma_gain"] - g) <= 1e-12 * g and abs(s2["keypoints"]["inliers"]["rms_z"] - 1) <= 1e-12
    # the marginal blocks are 3 dof each: within six standard errors of 3 (variance 6)
    for v in s2["pose"]["mean_nees"][1:]:
        assert abs(v - 3) <= 6 * math.sqrt(6 / N_STAT)


def test_status_and_flag_rules():
    x, _ = _experiment()
    x = {k: (v[:8].copy() if isinstance(v, np.ndarray) and v.shape[:1] == (N_STAT,) else v) for k, v in x.items()}
    x["q_gt"][0] = 0                                   # 1: ground truth unusable
    x["t_gt"][1, 2] = np.inf                           # 1
    x["status"][2] = 2                                 # 2: no pose
    x["cov_status"][3] = 2                             # 3: no covariance
    x["cov"][4] = 0                                    # 4: singular
    x["sigmas"][5, 0, 0] = np.nan                      # a keypoint without a sigma
    x["inlier_mask"][6] = 0x7FE                        # correspondence 0 is no inlier
    rec = cr.calibration_records(**x)
    assert rec["calib_status"].tolist() == [1, 1, 2, 3, 4, 0, 0, 0]
    assert not rec["z"][:2].any() and not rec["kp_flags"][:2].any() and not rec["delta"][:3].any()
    assert rec["delta"][3].any() and rec["delta"][4].any() and not rec["nees"][:5].any() and rec["nees"][5:].all()
    assert (rec["kp_flags"][2] == 1).all()             # valid, but no pose: no inliers
    l5 = int(x["probs"][5, 0].argmax())
    assert rec["kp_flags"][5, l5] == 2 and not rec["z"][5, l5].any() and (np.delete(rec["kp_flags"][5], l5) == 3).all()
    l6 = int(x["corr_label"][6, 0])
    assert rec["kp_flags"][6, l6] == 1 and (np.delete(rec["kp_flags"][6], l6) == 3).all()
    assert all(np.isfinite(rec[k]).all() for k in ("delta", "nees", "z"))


def test_pipeline_refuses_calibration_under_a_graph():
    """A graph replay runs no Python: the accumulator would hold two batches whatever ran.  Refused in the
    constructor, before the model or the device is touched."""
    from spe.pipeline import PosePipeline
    with pytest.raises(ValueError, match="eager"):
        PosePipeline(None, None, 4, use_graph=True, calibration=object())


def test_records_refuse_lens_poses_without_a_solver():
    import torch
    from spe.calibration import calibration_records
    z = torch.zeros(1, 11, 2)
    with pytest.raises(ValueError, match="lens"):
        calibration_records(z, torch.zeros(1, 11, 12), z, {"points_ideal": z}, {}, None, None)


def test_abi_exports_calibration_records():
    import os
    import re
    from conftest import REPO
    from spe import _lib
    L = _lib.lib()
    assert "spe_calibration_records" in _lib.EXPORTS and hasattr(L, "spe_calibration_records")
    assert len(L.spe_calibration_records.argtypes) == 26
    assert re.search(r"^int spe_calibration_records\(", open(os.path.join(REPO, "include", "spe.h")).read(), re.M)
    assert L.spe_abi_version() == _lib.ABI_VERSION == 9
