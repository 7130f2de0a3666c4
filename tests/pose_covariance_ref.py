"""numpy fp64 restatement of the pose covariance (include/spe.h spe_pose_covariance), written from the
definition and not from the kernel: plain matrix products, numpy's inverse, no fixed summation tree.
The selected correspondences come from oracle/pnp_ref.select_correspondences (the reference's
selection: best-score query per label, the first on ties), which is handed the sigmas in place of the
points and so returns each label's selected sigma.

Also here: the projection the Jacobian differentiates, a Gauss-Newton re-solve for the Monte-Carlo
check, and the synthetic inputs that tests/test_pose_covariance.py and
tests/test_gpu_pose_covariance.py share.
"""
import numpy as np

import pnp_ref
from spe.config import Camera, world_points

EPS = np.finfo(np.float64).eps
PIVOT_MIN = 64 * EPS
MAXN = 16


def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < EPS:
        return np.eye(3)
    k = r / th
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * hat(k)


def project(R, t, X, K):
    """Pixels of the world points X [n,3] under (R, t)."""
    Xc = X @ R.T + t
    return np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)


def perturbed(R, t, d):
    """The definition's perturbation: R <- exp([dw]x) R, t <- t + dt."""
    return rodrigues(d[:3]) @ R, t + d[3:]


def jacobian(R, t, X, K):
    """d pixel / d (dw, dt) at zero perturbation for one world point: 2x6."""
    RX = R @ X
    x, y, z = RX + t
    fx, fy = K[0, 0], K[1, 1]
    A = np.array([[fx / z, 0, -fx * x / z ** 2], [0, fy / z, -fy * y / z ** 2]])
    return A @ np.hstack([-hat(RX), np.eye(3)])


def selected_sigmas(probs_b, sigmas_b):
    """label -> the selected query's sigma [2] (float32 values), through pnp_ref's selection."""
    labs, sel = pnp_ref.select_correspondences(np.asarray(sigmas_b, np.float32), probs_b)
    return {int(l): sel[i] for i, l in enumerate(labs)}


def scaled_information(H):
    d = np.diag(H)
    s = 1.0 / np.sqrt(d)
    return H * np.outer(s, s), s


def pivots(S):
    """The Cholesky pivots of S in order, up to and including the first one <= PIVOT_MIN."""
    n = len(S)
    L = np.zeros_like(S)
    out = []
    for j in range(n):
        p = S[j, j] - L[j, :j] @ L[j, :j]
        out.append(p)
        if not p > PIVOT_MIN:
            break
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return out


def pose_covariance(probs, sigmas, status, corr_label, inlier_mask, rvec, tvec, K, world, sigma_scale=None,
                    sigma_floor=1e-3):
    """-> dict(cov [B,6,6], sigma_rot [B], sigma_t [B,3], pred_score [B], cov_status [B] int32, kappa [B]: the
    condition number of the scaled information matrix, nan where it was not formed, min_pivot [B], H [B,6,6]:
    the information matrix of the status-0 images)."""
    assert sigma_floor > 0
    B, Q, C = probs.shape
    K = np.asarray(K, np.float64)
    world = np.asarray(world, np.float64)
    o = dict(cov=np.zeros((B, 6, 6)), sigma_rot=np.zeros(B), sigma_t=np.zeros((B, 3)), pred_score=np.zeros(B),
             cov_status=np.zeros(B, np.int32), H=np.zeros((B, 6, 6)), kappa=np.full(B, np.nan), min_pivot=np.full(B, np.nan))
    for b in range(B):
        if int(status[b]) not in (0, 3):
            o["cov_status"][b] = 1
            continue
        sel = selected_sigmas(probs[b], sigmas[b])
        scale = np.ones(2) if sigma_scale is None else np.asarray(sigma_scale[b], np.float32).astype(np.float64)
        X, sg = [], []
        for i in range(MAXN):
            lab = int(corr_label[b, i])
            if (int(inlier_mask[b]) >> i) & 1 and 0 <= lab < C - 1 and lab in sel:
                X.append(world[lab])
                sg.append(sel[lab].astype(np.float64) * scale)
        if len(X) < 3:
            o["cov_status"][b] = 2
            continue
        X, sg = np.array(X), np.array(sg)
        if not np.isfinite(sg).all():
            o["cov_status"][b] = 3
            continue
        sg = np.maximum(sg, np.float64(np.float32(sigma_floor)))
        R, t = rodrigues(rvec[b]), np.asarray(tvec[b], np.float64)
        z = (X @ R.T + t)[:, 2]
        if not (z > 0).all():
            o["cov_status"][b] = 4
            continue
        H = np.zeros((6, 6))
        for Xi, si in zip(X, sg):
            J = jacobian(R, t, Xi, K)
            H += J.T @ np.diag(1.0 / si ** 2) @ J
        d = np.diag(H)
        if not (np.all(d > 0) and np.isfinite(d).all()):
            o["cov_status"][b] = 4
            continue
        S, s = scaled_information(H)
        pv = pivots(S)
        o["min_pivot"][b] = min(pv)
        if len(pv) < 6 or not pv[-1] > PIVOT_MIN:
            o["cov_status"][b] = 4
            continue
        o["kappa"][b] = np.linalg.cond(S)
        cov = np.linalg.inv(S) * np.outer(s, s)
        cov = 0.5 * (cov + cov.T)
        tn = np.linalg.norm(t)
        with np.errstate(divide="ignore", invalid="ignore"):
            pred = np.sqrt(np.trace(cov[:3, :3])) + np.sqrt(np.trace(cov[3:, 3:])) / tn
        if not (np.isfinite(cov).all() and np.isfinite(pred)):
            o["cov_status"][b] = 4
            continue
        o["cov"][b] = cov
        o["H"][b] = H
        o["sigma_rot"][b] = np.sqrt(np.trace(cov[:3, :3]))
        o["sigma_t"][b] = np.sqrt(np.diag(cov)[3:])
        o["pred_score"][b] = pred
    return o


def gauss_newton(R, t, X, uv, sg, K, steps=4):
    """Weighted least squares of the reprojection error from (R, t): `steps` Gauss-Newton steps in the
    definition's parametrisation.  -> the total perturbation (dw, dt) composed to first order exactly:
    the returned pose is (R1, t1) and the 6-vector is (log(R1 R^T), t1 - t)."""
    R1, t1 = R.copy(), t.copy()
    w = (1.0 / sg ** 2).reshape(-1)
    for _ in range(steps):
        J = np.vstack([jacobian(R1, t1, Xi, K) for Xi in X])
        r = (uv - project(R1, t1, X, K)).reshape(-1)
        d = np.linalg.solve(J.T @ (w[:, None] * J), J.T @ (w * r))
        R1, t1 = perturbed(R1, t1, d)
    dR = R1 @ R.T
    ang = np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))
    ax = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    dw = ax * (0.5 if ang < 1e-12 else ang / (2 * np.sin(ang)))
    return np.concatenate([dw, t1 - t])


# ---------------------------------------------------------------- shared synthetic inputs
def quat_to_R(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def keypoint_set(B, Q, C, world, K, seed, noise=0.3, spread=8.0):
    """B images of Q queries: the first min(Q, C - 1) queries carry the labels in a random order, on their
    projection + N(0, noise px); the remaining queries are background, except that in every image one
    extra query (when Q allows) repeats a present label with a bit-identical score and a point 40 px off --
    the tie the selection must give to the earlier query.  sigmas: an image's level is log-uniform in
    [1e-3, 1e2 / spread] and each keypoint and axis multiplies it by a log-uniform factor in [1, spread]:
    anisotropic, the whole range 1e-3 .. 1e2 over a batch, and a weight ratio of at most spread^2 inside one
    image (the scaled information matrix's condition number grows with it).  -> points [B,Q,2] f32, probs [B,Q,C] f32, sigmas [B,Q,2] f32, R [B,3,3], t [B,3]."""
    rng = np.random.default_rng(seed)
    world = np.asarray(world, np.float64)
    n = min(Q, C - 1)
    pts = np.zeros((B, Q, 2), np.float32)
    probs = np.full((B, Q, C), 0.01, np.float32)
    Rs, ts = np.zeros((B, 3, 3)), np.zeros((B, 3))
    level = np.exp(rng.uniform(np.log(1e-3), np.log(1e2 / spread), (B, 1, 1)))
    sig = (level * np.exp(rng.uniform(0, np.log(spread), (B, Q, 2)))).astype(np.float32)
    for b in range(B):
        R = quat_to_R(rng.normal(size=4))
        t = np.array([rng.normal(0, .3), rng.normal(0, .3), rng.uniform(4, 12)])
        Rs[b], ts[b] = R, t
        labels = np.full(Q, C - 1)
        labels[:n] = rng.permutation(C - 1)[:n]
        uv = project(R, t, world[np.minimum(labels, C - 2)], K) + rng.normal(0, noise, (Q, 2))
        hi = rng.uniform(0.6, 0.85, Q).astype(np.float32)
        if Q > n:                                        # the tied duplicate, later in the row order
            src = int(rng.integers(n))
            labels[n] = labels[src]
            hi[n] = hi[src]
            uv[n] = uv[src] + 40.0
        probs[b, np.arange(Q), labels] = hi
        pts[b] = uv.astype(np.float32)
    return pts, probs, sig, Rs, ts


def doctor_masks(mask, n_corr, counts, seed):
    """Force the inlier counts `counts` (cycled over the images that have at least that many
    correspondences) by keeping random subsets of each image's correspondences."""
    rng = np.random.default_rng(seed)
    out = np.array(mask, np.uint32).copy()
    for b in range(len(out)):
        want = counts[b % len(counts)]
        if n_corr[b] >= want:
            keep = rng.choice(int(n_corr[b]), want, replace=False)
            out[b] = np.uint32(sum(1 << int(i) for i in keep))
    return out


# ---------------------------------------------------------------- hand-built single images (11 landmarks)
K = Camera.K
W = world_points()
C = len(W) + 1


def pose(seed, z=10.0):
    rng = np.random.default_rng(seed)
    R = quat_to_R(rng.normal(size=4))
    t = np.array([rng.normal(0, .3), rng.normal(0, .3), z])
    return R, t


def rvec_of(R):
    ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return ax * (ang / (2 * np.sin(ang)))


def one_image(R, t, sig, labels=None, mask=None, status=0, corr=None):
    """Solver-shaped inputs of one image whose query q carries label labels[q] (default q); corr: the
    correspondences' labels in place of the first-seen order."""
    labels = np.arange(C - 1) if labels is None else np.asarray(labels)
    Q = len(labels)
    probs = np.full((1, Q, C), 0.01, np.float32)
    probs[0, np.arange(Q), labels] = 0.8
    seen = list(dict.fromkeys(int(l) for l in labels if l != C - 1)) if corr is None else list(corr)
    corr = np.full((1, 16), -1, np.int32)
    corr[0, :len(seen)] = seen
    m = (1 << len(seen)) - 1 if mask is None else mask
    return dict(probs=probs, sigmas=np.asarray(sig, np.float32).reshape(1, Q, 2), status=np.array([status], np.int32),
                corr_label=corr, inlier_mask=np.array([m], np.uint32), rvec=rvec_of(R)[None], tvec=t[None].copy(),
                K=K, world=W)


def status_cases():
    """name -> (inputs of one image, expected cov_status): every rule of the definition."""
    R, t = pose(5, z=8.0)
    sig = np.full((C - 1, 2), 0.5, np.float32)
    cases = {"ok": (one_image(R, t, sig), 0),
             "ok_fallback_status": (one_image(R, t, sig, status=3), 0),
             "no_pose": (one_image(R, t, sig, status=2), 1),
             "two_inliers": (one_image(R, t, sig, mask=0b101), 2)}
    bad = sig.copy()
    bad[3, 1] = np.inf
    cases["inf_sigma"] = (one_image(R, t, bad), 3)
    bad = sig.copy()
    bad[0, 0] = np.nan
    cases["nan_sigma"] = (one_image(R, t, bad), 3)
    # a non-finite sigma on a correspondence that is no inlier does not count
    cases["nan_sigma_outlier"] = (one_image(R, t, bad, mask=0x7FE), 0)
    # every inlier the same landmark (doctored labels): one world point, rank 2
    cases["one_world_point"] = (one_image(R, t, sig, corr=[4] * 6), 4)
    behind = one_image(R, np.array([0.0, 0.0, 0.2]), sig)    # the landmarks reach +-0.6 m: some z <= 0
    cases["behind_camera"] = (behind, 4)
    return cases
