"""numpy fp64 restatement of the calibration records and their summary (include/spe.h
spe_calibration_records, spe/calibration.py), written from the definition and not from the kernel: the
rotation error through rotation matrices and the quaternion read off R_pr R_gt^T, the NEES through
numpy's solve of the scaled matrix, the summary through plain sorts and loops.  The selection comes from
oracle/pnp_ref.select_correspondences, as in tests/pose_covariance_ref.py.

Also here: the synthetic statistical experiment tests/test_calibration.py and
tests/test_gpu_calibration.py share (keypoints = ground-truth projection + g * sigma Gaussian noise).
"""
import math

import numpy as np

import pnp_ref
import pose_covariance_ref as pc

EPS = np.finfo(np.float64).eps
PIVOT_MIN = 64 * EPS
MAXN = 16

# chi-square quantiles at 50 / 90 / 99 %: the roots of the closed-form distribution functions below,
# found by bisection to the last bit (tests/test_calibration.py evaluates the functions at them)
CHI2_6 = (5.34812062744712, 10.64464067566842, 16.811893829770916)
CHI2_3 = (2.3659738843753377, 6.2513886311703235, 11.344866730144357)
NORMAL_COVERAGE = (0.6826894921370859, 0.9544997361036416, 0.9973002039367398)   # erf(k / sqrt 2), k = 1, 2, 3


def chi2_cdf(x, dof):
    if dof == 6:
        return 1 - math.exp(-x / 2) * (1 + x / 2 + x * x / 8)
    assert dof == 3
    return math.erf(math.sqrt(x / 2)) - math.sqrt(2 * x / math.pi) * math.exp(-x / 2)


def rotation_log(Rrel):
    """Log of a rotation matrix through its unit quaternion (w, v), w >= 0: 2 atan2(|v|, w) v / |v|.  The
    quaternion is read off the matrix by the branch with the largest pivot, so a small angle takes
    v = (skew part) / (4 w): no arccos anywhere."""
    t = np.trace(Rrel)
    if t > 0:
        w = 0.5 * np.sqrt(1 + t)
        v = np.array([Rrel[2, 1] - Rrel[1, 2], Rrel[0, 2] - Rrel[2, 0], Rrel[1, 0] - Rrel[0, 1]]) / (4 * w)
    else:
        i = int(np.argmax(np.diag(Rrel)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2 * np.sqrt(1 + Rrel[i, i] - Rrel[j, j] - Rrel[k, k])
        v = np.zeros(3)
        v[i] = 0.25 * s
        v[j] = (Rrel[j, i] + Rrel[i, j]) / s
        v[k] = (Rrel[k, i] + Rrel[i, k]) / s
        w = (Rrel[k, j] - Rrel[j, k]) / s
        if w < 0:
            w, v = -w, -v
    n = np.linalg.norm(v)
    return np.zeros(3) if n == 0 else v * (2 * np.arctan2(n, w) / n)


def pose_error(R_pr, t_pr, q_gt, t_gt):
    """(dw, dt) with R_pr = exp([dw]x) R_gt, t_pr = t_gt + dt."""
    R_gt = pc.quat_to_R(np.asarray(q_gt, np.float64))
    return np.concatenate([rotation_log(R_pr @ R_gt.T), np.asarray(t_pr, np.float64) - np.asarray(t_gt, np.float64)])


def scaled(S):
    s = 1.0 / np.sqrt(np.diag(S))
    return S * np.outer(s, s), s


def nees_of(S, d):
    """d^T S^-1 d by a solve of the Jacobi-scaled matrix; None where the definition's tests fail.  Also the
    scaled matrix's condition number."""
    dg = np.diag(S)
    if not (np.all(dg > 0) and np.isfinite(dg).all()):
        return None, np.nan
    A, s = scaled(S)
    pv = pc.pivots(A)
    if len(pv) < len(A) or not pv[-1] > PIVOT_MIN:
        return None, np.nan
    b = d * s
    v = float(b @ np.linalg.solve(A, b))
    return (v if np.isfinite(v) else None), float(np.linalg.cond(A))


def calibration_records(points, probs, sigmas, status, corr_label, inlier_mask, rvec, tvec, q_gt, t_gt, cov,
                        cov_status, K, world, sigma_scale=None, sigma_floor=1e-3, sigma_gain=1.0):
    """-> dict(delta [B,6], nees [B,3], z [B,L,2], kp_flags [B,L] u8, calib_status [B] i32, kappa [B,3]: the
    condition numbers of the three scaled matrices, nan where they were not formed)."""
    B, Q, C = probs.shape
    L = C - 1
    K = np.asarray(K, np.float64)
    world = np.asarray(world, np.float64)
    floor = np.float64(np.float32(sigma_floor))
    o = dict(delta=np.zeros((B, 6)), nees=np.zeros((B, 3)), z=np.zeros((B, L, 2)), kp_flags=np.zeros((B, L), np.uint8),
             calib_status=np.zeros(B, np.int32), kappa=np.full((B, 3), np.nan))
    for b in range(B):
        q = np.asarray(q_gt[b], np.float64)
        qn = np.sqrt((q * q).sum())
        if not (qn > 0 and np.isfinite(qn) and np.isfinite(t_gt[b]).all()):
            o["calib_status"][b] = 1
            continue
        R_gt, tg = pc.quat_to_R(q), np.asarray(t_gt[b], np.float64)
        have_pose = int(status[b]) in (0, 3)
        labs, sel_p = pnp_ref.select_correspondences(np.asarray(points[b], np.float32), probs[b])
        _, sel_s = pnp_ref.select_correspondences(np.asarray(sigmas[b], np.float32), probs[b])
        where = {int(l): i for i, l in enumerate(labs)}
        scale = np.ones(2) if sigma_scale is None else np.asarray(sigma_scale[b], np.float32).astype(np.float64)
        inl_labels = set()
        if have_pose:
            for i in range(MAXN):
                if (int(inlier_mask[b]) >> i) & 1:
                    inl_labels.add(int(corr_label[b, i]))
        for l in range(L):
            if l not in where:
                continue
            flags = 2 if l in inl_labels else 0
            p = sel_p[where[l]].astype(np.float64)
            sg = sel_s[where[l]].astype(np.float64) * scale * sigma_gain
            Xc = R_gt @ world[l] + tg
            if Xc[2] > 0 and np.isfinite(p).all() and np.isfinite(sg).all():
                uv = np.array([K[0, 0] * Xc[0] / Xc[2] + K[0, 2], K[1, 1] * Xc[1] / Xc[2] + K[1, 2]])
                with np.errstate(over="ignore", invalid="ignore"):
                    zz = (p - uv) / np.maximum(sg, floor)
                if np.isfinite(zz).all():
                    o["z"][b, l] = zz
                    flags |= 1
            o["kp_flags"][b, l] = flags
        if not have_pose:
            o["calib_status"][b] = 2
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            d = pose_error(pc.rodrigues(rvec[b]), tvec[b], q, tg)
        fin = bool(np.isfinite(d).all())
        o["delta"][b] = d if fin else 0
        if int(cov_status[b]) != 0:
            o["calib_status"][b] = 3
            continue
        if not fin:
            o["calib_status"][b] = 4
            continue
        S = np.asarray(cov[b], np.float64) * (sigma_gain * sigma_gain)
        parts = [nees_of(S, d), nees_of(S[:3, :3], d[:3]), nees_of(S[3:, 3:], d[3:])]
        if any(p[0] is None for p in parts):
            o["calib_status"][b] = 4
            continue
        o["nees"][b] = [p[0] for p in parts]
        o["kappa"][b] = [p[1] for p in parts]
    return o


# ---------------------------------------------------------------- the summary
def keypoint_stats(z, mask):
    """z [N,L,2], mask [N,L] bool -> the summary of the masked keypoints' 2 * count axis samples."""
    zz = z[mask]
    n = int(len(zz))
    if n == 0:
        return dict(count=0, mean_z=[0.0, 0.0], rms_z=0.0, mean_abs_z=0.0, coverage_count=[0, 0, 0],
                    coverage=[0.0, 0.0, 0.0])
    cc = [int((np.abs(zz) <= k).sum()) for k in (1, 2, 3)]
    return dict(count=n, mean_z=(zz.sum(0) / n).tolist(), rms_z=float(np.sqrt((zz * zz).sum() / (2 * n))),
                mean_abs_z=float(np.abs(zz).sum() / (2 * n)), coverage_count=cc, coverage=[c / (2 * n) for c in cc])


def order_desc(v):
    """Indices by value descending, the image index ascending on ties."""
    return sorted(range(len(v)), key=lambda i: (-v[i], i))


def sparsification(pred, score, steps=20):
    """The curves over the N images given: the mean true score of what remains after removing the worst
    floor(k N / steps) images, k = 0 .. steps - 1, by predicted score, by true score (oracle) and in no order;
    AUSE (trapezoid area between the first two over the removed fraction k / steps, over the mean score) and
    Spearman's rank correlation of the two orders (ranks from the stable orders: no tied ranks)."""
    pred, score = [float(x) for x in pred], [float(x) for x in score]
    N = len(pred)
    if N == 0:
        return dict(count=0, fractions=[k / steps for k in range(steps)], by_pred=[0.0] * steps, oracle=[0.0] * steps,
                    random=[0.0] * steps, ause=0.0, spearman=0.0)
    op, oo = order_desc(pred), order_desc(score)
    curves = {}
    for name, order in (("by_pred", op), ("oracle", oo)):
        c = []
        for k in range(steps):
            kept = order[(k * N) // steps:]
            c.append(math.fsum(score[i] for i in kept) / len(kept))
        curves[name] = c
    mean = math.fsum(score) / N
    diff = [a - b for a, b in zip(curves["by_pred"], curves["oracle"])]
    area = sum(0.5 * (diff[k] + diff[k + 1]) / steps for k in range(steps - 1))
    rp, ro = [0] * N, [0] * N
    for r, i in enumerate(op):
        rp[i] = r
    for r, i in enumerate(oo):
        ro[i] = r
    d2 = sum((a - b) ** 2 for a, b in zip(rp, ro))
    rho = 1.0 - 6.0 * d2 / (N * (N * N - 1)) if N > 1 else 0.0
    return dict(count=N, fractions=[k / steps for k in range(steps)], by_pred=curves["by_pred"], oracle=curves["oracle"],
                random=[mean] * steps, ause=(area / mean if mean > 0 else 0.0), spearman=rho)


def threshold_for(pred, score, risk):
    """The largest threshold t among the predicted scores whose kept set {pred <= t} has a mean true score
    <= risk, and the kept fraction: (None, 0.0) when no threshold qualifies."""
    pred, score = [float(x) for x in pred], [float(x) for x in score]
    best = (None, 0.0)
    for t in sorted(set(pred)):
        kept = [s for p, s in zip(pred, score) if p <= t]
        if math.fsum(kept) / len(kept) <= risk:
            best = (t, len(kept) / len(pred))
    return best


def summarize(rec, score, pred_score, cov_status, sigma_gain=1.0):
    """rec: calibration_records' dict over all images; score, pred_score, cov_status [N]."""
    valid = (rec["kp_flags"] & 1) != 0
    inl = valid & ((rec["kp_flags"] & 2) != 0)
    kp_all, kp_inl = keypoint_stats(rec["z"], valid), keypoint_stats(rec["z"], inl)
    ok = rec["calib_status"] == 0
    n = int(ok.sum())
    ne = rec["nees"][ok]
    mean_nees = (ne.sum(0) / n).tolist() if n else [0.0, 0.0, 0.0]
    below = {}
    for name, col, qs in (("full", 0, CHI2_6), ("rot", 1, CHI2_3), ("trans", 2, CHI2_3)):
        cnt = [int((ne[:, col] <= q).sum()) for q in qs]
        below[name] = dict(count=cnt, share=[c / n if n else 0.0 for c in cnt])
    keep = np.asarray(cov_status) == 0
    return dict(gain_in_force=float(sigma_gain),
                keypoints=dict(all=kp_all, inliers=kp_inl),
                sigma_gain=kp_inl["rms_z"] * sigma_gain,
                pose=dict(count=n, mean_nees=mean_nees, below_chi2=below,
                          cov_gain=float(np.sqrt(mean_nees[0] / 6.0)) * sigma_gain),
                status_count=[int((rec["calib_status"] == s).sum()) for s in range(5)],
                sparsification=sparsification(np.asarray(pred_score)[keep], np.asarray(score)[keep]))


# ---------------------------------------------------------------- the statistical experiment
G_TRUE = 2.0            # the keypoint noise is G_TRUE times the predicted sigma
NOISE_SEED = 20261


def experiment_inputs(N, seed=NOISE_SEED, g=G_TRUE, Q=11, per_image_sigma=False):
    """N images at SPEED-like ranges (z in [4, 12] m, as pose_covariance_ref.keypoint_set), the 11 landmarks
    in a random query order, and keypoints = the ground-truth projection + N(0, (g sigma)^2) per axis.  The
    predicted sigmas are log-uniform in [0.2, 0.8] px, drawn per keypoint and axis, or once per image
    (per_image_sigma): the device solver's LM weighs a residual by 1 / sqrt(sigma) as the reference does, which
    is the maximum-likelihood weighting the covariance describes only where an image's sigmas are equal, so the
    device loop draws them per image; the CPU re-solve weighs by 1 / sigma^2 and takes either.  The noise sigma
    is at most 1.6 px: the sigma solver's 25 px reprojection threshold is over 15 noise sigmas, no inlier is
    truncated.  -> points, probs, sigmas (float32), q_gt [N,4], t_gt [N,3], R [N,3,3]."""
    rng = np.random.default_rng(seed)
    world, K = pc.W, pc.K
    C = len(world) + 1
    pts = np.zeros((N, Q, 2), np.float32)
    probs = np.full((N, Q, C), 0.01, np.float32)
    shape = (N, 1, 1) if per_image_sigma else (N, Q, 2)
    sig = np.broadcast_to(np.exp(rng.uniform(np.log(0.2), np.log(0.8), shape)), (N, Q, 2)).astype(np.float32)
    q_gt, t_gt, Rs = np.zeros((N, 4)), np.zeros((N, 3)), np.zeros((N, 3, 3))
    for b in range(N):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        R = pc.quat_to_R(q)
        t = np.array([rng.normal(0, .3), rng.normal(0, .3), rng.uniform(4, 12)])
        labels = rng.permutation(C - 1)[:Q]
        uv = pc.project(R, t, world[labels], K) + rng.normal(size=(Q, 2)) * (g * sig[b].astype(np.float64))
        probs[b, np.arange(Q), labels] = rng.uniform(0.6, 0.85, Q).astype(np.float32)
        pts[b] = uv.astype(np.float32)
        q_gt[b], t_gt[b], Rs[b] = q, t, R
    return pts, probs, sig, q_gt, t_gt, Rs


def gauss_newton_pose(R, t, X, uv, sg, K, steps=3):
    """tests/pose_covariance_ref.gauss_newton's iteration, returning the pose."""
    R1, t1 = R.copy(), t.copy()
    w = (1.0 / sg ** 2).reshape(-1)
    for _ in range(steps):
        J = np.vstack([pc.jacobian(R1, t1, Xi, K) for Xi in X])
        r = (uv - pc.project(R1, t1, X, K)).reshape(-1)
        d = np.linalg.solve(J.T @ (w[:, None] * J), J.T @ (w * r))
        R1, t1 = pc.perturbed(R1, t1, d)
    return R1, t1


def rvec_of(R):
    return rotation_log(R)


def gates(N, L=11):
    """The statistical gates of the issue for N images of L landmarks: sigma_gain in g (1 +- 6 / sqrt(2 n)), n = 2 L N
    axis samples (the standard error of an rms of n unit normals is 1 / sqrt(2 n)); mean NEES in
    6 +- 6 sqrt(12 / N) (a chi-square of 6 dof has variance 12); coverage within six binomial standard errors."""
    n = 2 * L * N
    return dict(sigma_gain=(G_TRUE * (1 - 6 / math.sqrt(2 * n)), G_TRUE * (1 + 6 / math.sqrt(2 * n))),
                mean_nees=(6 - 6 * math.sqrt(12 / N), 6 + 6 * math.sqrt(12 / N)),
                coverage=[(p - 6 * math.sqrt(p * (1 - p) / n), p + 6 * math.sqrt(p * (1 - p) / n)) for p in NORMAL_COVERAGE])
