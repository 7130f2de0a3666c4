"""numpy fp64 restatement of include/spe.h's landmark reconstruction (spe_landmarks_solve,
spe_landmark_observations): the per-view arithmetic step by step as the header states it, the sums over
views by numpy in the order `order` gives them (the device's own order is a third one; the GPU test's
tolerance is measured from two orders here)."""
import numpy as np

EPS = np.finfo(np.float64).eps
THR = 64.0 * EPS


def rotations(q, t):
    """-> R [N,3,3] (zeros where unusable), ok [N]"""
    q = np.asarray(q, np.float64)
    t = np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        qn = np.sqrt(n2)
        ok = (qn > 0) & np.isfinite(qn) & np.isfinite(t).all(1)
        qs = np.where(ok[:, None], q / np.where(ok, qn, 1.0)[:, None], 0.0)
    w, x, y, z = qs.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    R[~ok] = 0.0
    return R, ok


def chol3_factor(S, thr):
    L = np.zeros((3, 3))
    for j in range(3):
        s = S[j, j]
        for p in range(j):
            s -= L[j, p] * L[j, p]
        if not s > thr:
            return None
        L[j, j] = np.sqrt(s)
        inv = 1.0 / L[j, j]
        for i in range(j + 1, 3):
            t = S[i, j]
            for p in range(j):
                t -= L[i, p] * L[j, p]
            L[i, j] = t * inv
    return L


def chol3_backsolve(L, b):
    y = np.zeros(3)
    x = np.zeros(3)
    for i in range(3):
        t = b[i]
        for p in range(i):
            t -= L[i, p] * y[p]
        y[i] = t / L[i, i]
    for i in (2, 1, 0):
        t = y[i]
        for p in range(i + 1, 3):
            t -= L[p, i] * x[p]
        x[i] = t / L[i, i]
    return x


def scaled_factor(H, lam):
    """Cholesky of D^-1/2 H D^-1/2 + lam I -> (L, scale) or None"""
    d = np.diag(H)
    if not (np.all(d > 0) and np.all(np.isfinite(d))):
        return None
    sc = 1.0 / np.sqrt(d)
    A = (H * sc[:, None]) * sc[None, :] + lam * np.eye(3)
    L = chol3_factor(A, THR)
    return None if L is None else (L, sc)


def scaled_solve(f, b):
    L, sc = f
    return chol3_backsolve(L, b * sc) * sc


def sym(u6):
    return np.array([[u6[0], u6[1], u6[2]], [u6[1], u6[3], u6[4]], [u6[2], u6[4], u6[5]]])


def _evaluate(R, t, K, p, s, X, huber, z_min):
    """per view of one landmark at X: used [n], beyond [n], terms [n,12] (H6, g3, rho, 1, px^2)"""
    with np.errstate(all="ignore"):
        xc = (R[:, 0, 0] * X[0] + R[:, 0, 1] * X[1] + R[:, 0, 2] * X[2]) + t[:, 0]
        yc = (R[:, 1, 0] * X[0] + R[:, 1, 1] * X[1] + R[:, 1, 2] * X[2]) + t[:, 1]
        zc = (R[:, 2, 0] * X[0] + R[:, 2, 1] * X[1] + R[:, 2, 2] * X[2]) + t[:, 2]
        xz, yz = xc / zc, yc / zc
        ex = p[:, 0] - (K[0, 0] * xz + K[0, 2])
        ey = p[:, 1] - (K[1, 1] * yz + K[1, 2])
        rx, ry = ex / s[:, 0], ey / s[:, 1]
        s2 = rx * rx + ry * ry
        nr = np.sqrt(s2)
        used = (zc > z_min) & np.isfinite(nr)
        beyond = used & (huber > 0) & (nr > huber)
        w = np.where(beyond, huber / nr, 1.0)
        rho = np.where(beyond, 2.0 * huber * nr - huber * huber, s2)
        ax, ay = (K[0, 0] / zc) / s[:, 0], (K[1, 1] / zc) / s[:, 1]
        jx = ax[:, None] * (R[:, 0, :] - xz[:, None] * R[:, 2, :])
        jy = ay[:, None] * (R[:, 1, :] - yz[:, None] * R[:, 2, :])
        T = np.zeros((len(p), 12))
        for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            T[:, k] = w * (jx[:, i] * jx[:, j] + jy[:, i] * jy[:, j])
        for i in range(3):
            T[:, 6 + i] = w * (jx[:, i] * rx + jy[:, i] * ry)
        T[:, 9] = rho
        T[:, 10] = 1.0
        T[:, 11] = ex * ex + ey * ey
    T[~used] = 0.0
    return used, beyond, T


def _linear(R, t, K, p, s):
    f = (K[0, 0], K[1, 1])
    uv = ((p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1])
    T = np.zeros((len(p), 12))
    for r in range(2):
        q = f[r] / s[:, r]
        w = q * q
        c = R[:, r, :] - uv[r][:, None] * R[:, 2, :]
        b = -(t[:, r] - uv[r] * t[:, 2])
        wc = w[:, None] * c
        for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            T[:, k] += wc[:, i] * c[:, j]
        for i in range(3):
            T[:, 6 + i] += wc[:, i] * b
    T[:, 10] = 1.0
    return T


def solve(obs_px, obs_sigma, obs_valid, q_gt, t_gt, K, world_init=None, iterations=10, huber=3.0,
          sigma_floor=1e-3, sigma_gain=1.0, z_min=0.1, order=None):
    """-> dict world [L,3], cov [L,3,3], chi2, n_used, rms_px, status [L], obs_flags [N,L].  order: the
    permutation of the views the sums are taken in (None: as given)."""
    obs_px = np.asarray(obs_px, np.float64)
    N, L = obs_px.shape[:2]
    K = np.asarray(K, np.float64).reshape(3, 3)
    obs_valid = np.asarray(obs_valid).astype(bool)
    sig = np.ones((N, L, 2)) if obs_sigma is None else np.asarray(obs_sigma, np.float64)
    R, vok = rotations(q_gt, t_gt)
    t = np.where(vok[:, None], np.asarray(t_gt, np.float64), 0.0)
    order = np.arange(N) if order is None else np.asarray(order)
    out = dict(world=np.zeros((L, 3)), cov=np.zeros((L, 3, 3)), chi2=np.zeros(L), n_used=np.zeros(L, np.int32),
               rms_px=np.zeros(L), status=np.zeros(L, np.int32), obs_flags=np.zeros((N, L), np.uint8))
    for l in range(L):
        with np.errstate(all="ignore"):
            sg = sig[:, l] * sigma_gain
        cand = obs_valid[:, l] & vok & np.isfinite(obs_px[:, l]).all(1) & np.isfinite(sg).all(1)
        idx = order[cand[order]]
        p, s = obs_px[idx, l], np.maximum(sg[idx], sigma_floor)
        Rl, tl = R[idx], t[idx]
        status = 0
        # stage 0
        if world_init is not None:
            X = np.asarray(world_init, np.float64)[l].copy()
            if not np.isfinite(X).all():
                status = 3
        else:
            if len(idx) < 2:
                status = 1
            else:
                T = _linear(Rl, tl, K, p, s).sum(0)
                f = scaled_factor(sym(T[:6]), 0.0)
                if f is None:
                    status = 2
                else:
                    X = scaled_solve(f, T[6:9])
                    if not np.isfinite(X).all():
                        status = 3
        # stage 1
        acc = None
        lam = 1e-3
        for k in range(iterations + 1):
            if status:
                break
            used, beyond, Tv = _evaluate(Rl, tl, K, p, s, X, huber, z_min)
            T = Tv.sum(0)
            n = int(used.sum())
            if acc is None:
                if n < 2:
                    status = 1
                    break
                accept = True
            else:
                accept = bool(T[9] < acc["T"][9]) and n >= acc["n"]
                lam = lam / 10.0 if accept else lam * 10.0
            if accept:
                acc = dict(X=X.copy(), T=T, n=n, used=used, beyond=beyond)
            if k < iterations:
                f = scaled_factor(sym(acc["T"][:6]), lam)
                if f is None:
                    status = 2
                    break
                X = acc["X"] + scaled_solve(f, acc["T"][6:9])
                if not np.isfinite(X).all():
                    status = 3
        if not status:
            f = scaled_factor(sym(acc["T"][:6]), 0.0)
            if f is None:
                status = 2
            else:
                C = np.zeros((3, 3))
                for j in range(3):
                    col = scaled_solve(f, np.eye(3)[j])
                    for i in range(j + 1):
                        C[i, j] = C[j, i] = col[i]
                rms = np.sqrt(acc["T"][11] / acc["n"])
                if not (np.isfinite(C).all() and np.isfinite(acc["X"]).all() and np.isfinite(acc["T"][9])
                        and np.isfinite(rms)):
                    status = 3
        out["status"][l] = status
        if status:
            continue
        out["world"][l], out["cov"][l], out["chi2"][l] = acc["X"], C, acc["T"][9]
        out["n_used"][l], out["rms_px"][l] = acc["n"], rms
        out["obs_flags"][idx, l] = acc["used"].astype(np.uint8) | (acc["beyond"].astype(np.uint8) << 1)
    return out


def select_observations(points_px, probs, sigmas=None, sigma_scale=None):
    """spe_landmark_observations: -> obs_px [B,L,2] f64, obs_sigma [B,L,2] f64, obs_valid [B,L] u8"""
    points_px = np.asarray(points_px, np.float32)
    probs = np.asarray(probs, np.float32)
    B, Q, C = probs.shape
    L = C - 1
    px = np.zeros((B, L, 2))
    sg = np.ones((B, L, 2))
    valid = np.zeros((B, L), np.uint8)
    for b in range(B):
        lab = probs[b].argmax(1)                  # the first maximum, like argmax_class
        sc = probs[b].max(1)
        for l in range(L):
            best = -1
            for q in range(Q):
                if lab[q] == l and (best < 0 or sc[q] > sc[best]):
                    best = q
            if best < 0:
                continue
            valid[b, l] = 1
            px[b, l] = points_px[b, best].astype(np.float64)
            if sigmas is not None:
                s = np.asarray(sigmas, np.float32)[b, best].astype(np.float64)
                if sigma_scale is not None:
                    s = s * np.asarray(sigma_scale, np.float32)[b].astype(np.float64)
                sg[b, l] = s
    return px, sg, valid


def quat_of(R):
    """(w, x, y, z) of a rotation matrix, the inverse of rotations()"""
    tr = np.trace(R)
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0, 0, 0, 0]
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return np.asarray(q)


def synthetic_views(N, world, K, seed, noise=0.0, sigma=None):
    """N random poses in front of the camera with every landmark in view: q [N,4], t [N,3], the exact
    projections plus `noise` px gaussian noise times sigma [N,L,2] (None: 1)"""
    rng = np.random.default_rng(seed)
    L = len(world)
    q = rng.normal(size=(N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.stack([rng.uniform(-0.4, 0.4, N), rng.uniform(-0.3, 0.3, N), rng.uniform(4.0, 12.0, N)], 1)
    R, _ = rotations(q, t)
    Xc = np.einsum("nij,lj->nli", R, world) + t[:, None, :]
    px = np.stack([K[0, 0] * Xc[..., 0] / Xc[..., 2] + K[0, 2], K[1, 1] * Xc[..., 1] / Xc[..., 2] + K[1, 2]], -1)
    if noise:
        px = px + noise * rng.normal(size=(N, L, 2)) * (1.0 if sigma is None else sigma)
    return q, t, px


def model_outputs(N, world, K, seed, Q=None):
    """A stand-in model's output for N posed views, 1 sigma of noise: points_px [N,Q,2] f32, probs [N,Q,C] f32,
    crop-normalised sigmas [N,Q,2] f32, clip_bbox [N,4] f32 (x1, y1, x2, y2), and q [N,4], t [N,3].  Query l
    carries landmark l; queries beyond L are background."""
    rng = np.random.default_rng(seed)
    L = len(world)
    Q = L if Q is None else Q
    sigma_px = rng.uniform(0.5, 2.0, (N, L, 2))
    q, t, px = synthetic_views(N, world, K, seed + 1, noise=1.0, sigma=sigma_px)
    xy = rng.uniform(0, 600, (N, 2))
    wh = np.stack([rng.uniform(200, 400, N), rng.uniform(450, 700, N)], 1)
    clip = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    size = np.stack([clip[:, 2] - clip[:, 0], clip[:, 3] - clip[:, 1]], 1)          # fp32, as sigma_scale_of
    points = np.zeros((N, Q, 2), np.float32)
    sig = np.ones((N, Q, 2), np.float32)
    probs = np.full((N, Q, L + 1), 0.01, np.float32)
    probs[:, :, L] = 0.9
    points[:, :L] = px
    sig[:, :L] = sigma_px / size[:, None, :]
    probs[:, np.arange(L), L] = 0.01
    probs[:, np.arange(L), np.arange(L)] = 0.9
    return dict(points=points, probs=probs, sigmas=sig, clip=clip, scale=size, q=q, t=t)


def within_3_sigma(world, cov, chi2, n_used, truth):
    """per landmark: every coordinate within 3 sqrt(diag(cov * max(1, chi2 / (2 n - 3)))) of the truth"""
    birge = np.maximum(1.0, chi2 / np.maximum(2.0 * n_used - 3.0, 1.0))
    sd = np.sqrt(np.diagonal(cov, axis1=1, axis2=2) * birge[:, None])
    return (np.abs(world - truth) <= 3.0 * sd).all(1)
