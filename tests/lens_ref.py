"""numpy fp64 restatement of the lens model (include/spe.h spe_undistort_points / spe_distort_points),
written from the definition there: OpenCV's five-coefficient model dist = (k1, k2, p1, p2, k3), the
fixed-point undistortion run for exactly `iters` rounds, the closed-form Jacobian D of the distort map
in pixels and the per-axis sigma rule.  Every expression keeps the definition's order of operations, so
the kernel (compiled without contraction) is expected to agree to the last fp64 bits."""
import numpy as np

from spe.config import Camera

K = Camera.K.copy()
# calibration-like magnitudes (k1 ~ -0.22 as in SPEED+-class calibrations), not any dataset's file
DIST = np.array([-0.22383016606510672, 0.51409797089106379, -0.00066499611998340662,
                 -0.00021404771667484594, -0.13124227429077406])
MARGIN = 200.0          # px around the frame the test points cover


def _k(K):
    K = np.asarray(K, np.float64).reshape(3, 3)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def _d(dist):
    d = np.asarray(dist, np.float64).ravel()
    return d[0], d[1], d[2], d[3], d[4]


def distort_normalised(x, y, dist):
    k1, k2, p1, p2, k3 = _d(dist)
    r2 = x * x + y * y
    rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return xd, yd


def distort(points_ideal, K, dist):
    """ideal pixel points [...,2] -> distorted pixel points, fp64."""
    fx, fy, cx, cy = _k(K)
    p = np.asarray(points_ideal, np.float64)
    xd, yd = distort_normalised((p[..., 0] - cx) / fx, (p[..., 1] - cy) / fy, dist)
    return np.stack((fx * xd + cx, fy * yd + cy), -1)


def undistort(points_px, K, dist, iters=5):
    """distorted pixel points [...,2] -> (ideal pixel points fp64, status uint8, normalised x, y).
    status 1: icd not positive and finite in some round; the point is then returned unchanged."""
    fx, fy, cx, cy = _k(K)
    k1, k2, p1, p2, k3 = _d(dist)
    p = np.asarray(points_px, np.float64)
    x0, y0 = (p[..., 0] - cx) / fx, (p[..., 1] - cy) / fy
    x, y = x0.copy(), y0.copy()
    bad = np.zeros(x.shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(int(iters)):
            r2 = x * x + y * y
            icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            bad |= ~((icd > 0) & np.isfinite(icd))
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x = (x0 - dx) * icd
            y = (y0 - dy) * icd
    out = np.stack((fx * x + cx, fy * y + cy), -1)
    out[bad] = p[bad]
    return out, bad.astype(np.uint8), x, y


def jacobian(x, y, K, dist):
    """D = d(ud, vd) / d(ui, vi) at the ideal normalised point (x, y): D11, D12, D21, D22."""
    fx, fy, _, _ = _k(K)
    k1, k2, p1, p2, k3 = _d(dist)
    r2 = x * x + y * y
    rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    g = (3.0 * k3 * r2 + 2.0 * k2) * r2 + k1                # d rad / d r2
    c = 2.0 * x * y * g + 2.0 * p1 * x + 2.0 * p2 * y       # the normalised map's off-diagonal
    d11 = rad + 2.0 * x * x * g + 2.0 * p1 * y + 6.0 * p2 * x
    d22 = rad + 2.0 * y * y * g + 6.0 * p1 * y + 2.0 * p2 * x
    return d11, c * (fx / fy), c * (fy / fx), d22


def undistort_points(points_px, sigmas=None, sigma_scale=None, K=K, dist=DIST, iters=5):
    """spe_undistort_points on [B,Q,2] arrays -> dict(points float32, sigmas float32 or None, status
    uint8, points64, sigmas64).  All-zero dist: a copy."""
    p32 = np.asarray(points_px, np.float32)
    s32 = None if sigmas is None else np.asarray(sigmas, np.float32)
    if not np.any(np.asarray(dist, np.float64)):
        return dict(points=p32.copy(), sigmas=None if s32 is None else s32.copy(),
                    status=np.zeros(p32.shape[:-1], np.uint8), points64=p32.astype(np.float64),
                    sigmas64=None if s32 is None else s32.astype(np.float64))
    pts, bad, x, y = undistort(p32, K, dist, iters)
    with np.errstate(all="ignore"):
        d11, d12, d21, d22 = jacobian(x, y, K, dist)
        det = d11 * d22 - d12 * d21
        bad = (bad != 0) | ~((np.abs(det) > 0) & np.isfinite(det))
    pts[bad] = p32.astype(np.float64)[bad]
    sig = None
    if s32 is not None:
        sc = np.ones(p32.shape[:-2] + (1, 2)) if sigma_scale is None else \
            np.asarray(sigma_scale, np.float32).astype(np.float64)[..., None, :]
        sx, sy = sc[..., 0], sc[..., 1]
        ux, uy = s32[..., 0].astype(np.float64) * sx, s32[..., 1].astype(np.float64) * sy
        with np.errstate(all="ignore"):
            a11, a12, a21, a22 = d22 / det, -d12 / det, -d21 / det, d11 / det
            gx = np.sqrt((a11 * a11) * (ux * ux) + (a12 * a12) * (uy * uy)) / sx
            gy = np.sqrt((a21 * a21) * (ux * ux) + (a22 * a22) * (uy * uy)) / sy
        sig = np.stack((gx, gy), -1)
        sig[bad] = s32.astype(np.float64)[bad]
    return dict(points=pts.astype(np.float32), sigmas=None if sig is None else sig.astype(np.float32),
                status=bad.astype(np.uint8), points64=pts, sigmas64=sig)


def frame_grid(nx=117, ny=81, margin=MARGIN):
    """ideal pixel points on an nx x ny grid over the frame plus the margin, [ny*nx, 2] fp64."""
    u = np.linspace(-margin, Camera.nu + margin, nx)
    v = np.linspace(-margin, Camera.nv + margin, ny)
    return np.stack(np.meshgrid(u, v), -1).reshape(-1, 2)


def random_points(rng, shape, margin=MARGIN):
    """distorted pixel points drawn over the frame plus the margin, float32 [*shape, 2]."""
    lo = np.array([-margin, -margin])
    hi = np.array([Camera.nu + margin, Camera.nv + margin])
    return rng.uniform(lo, hi, tuple(shape) + (2,)).astype(np.float32)


def ulp_diff(a, b):
    """distance of two float32 arrays in units in the last place (finite values)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
