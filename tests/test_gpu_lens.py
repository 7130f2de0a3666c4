"""GPU: spe_undistort_points / spe_distort_points (csrc/lens.hip) against the numpy restatement
tests/lens_ref.py, and the lens threaded through the solver classes, the sigma ensemble and PosePipeline.

Tolerances.  The kernel and the restatement run the same fp64 steps in the same order (lens.hip is built
without contraction), so their fp64 results differ by a few fp64 ulps at most (division and sqrt are
correctly rounded on both sides); after the single rounding to float32 the two can differ only where the
fp64 value sits on a rounding boundary: 1 float32 ulp for the points, 1e-5 relative for the sigmas (a
float32 ulp is 1.2e-7 relative)."""
import numpy as np
import pytest
import torch

import lens_ref as lr
from spe import _lib
from spe.config import Camera, LensModel, project, quat_to_matrix, world_points

pytestmark = pytest.mark.gpu

K, DIST = lr.K, lr.DIST


def _dev64(a, dev):
    return torch.as_tensor(np.asarray(a, np.float64), dtype=torch.float64, device=dev).contiguous()


def _undistort(dev, p, s=None, scale=None, dist=DIST, iters=5, inplace=False):
    """spe_undistort_points on numpy arrays -> (points, sigmas or None, status) as numpy."""
    pt = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev)
    st = torch.from_numpy(np.ascontiguousarray(s, np.float32)).to(dev) if s is not None else None
    sc = torch.from_numpy(np.ascontiguousarray(scale, np.float32)).to(dev) if scale is not None else None
    B, Q = pt.shape[:2]
    po = pt if inplace else torch.full_like(pt, -7.0)
    so = None if st is None else (st if inplace else torch.full_like(st, -7.0))
    status = torch.full((B, Q), 9, dtype=torch.uint8, device=dev)
    Kd, dd = _dev64(K, dev), _dev64(dist, dev)              # named: they must outlive the launch
    _lib.check(_lib.lib().spe_undistort_points(
        _lib.stream_ptr(), _lib.ptr(pt), _lib.ptr(st), _lib.ptr(sc), B, Q, _lib.ptr(Kd), _lib.ptr(dd), iters,
        _lib.ptr(po), _lib.ptr(so), _lib.ptr(status)), "spe_undistort_points")
    torch.cuda.synchronize()
    return po.cpu().numpy(), None if so is None else so.cpu().numpy(), status.cpu().numpy()


def _distort(dev, p, dist=DIST):
    pt = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev)
    out = torch.full_like(pt, -7.0)
    B, Q = pt.shape[:2]
    Kd, dd = _dev64(K, dev), _dev64(dist, dev)
    _lib.check(_lib.lib().spe_distort_points(_lib.stream_ptr(), _lib.ptr(pt), B, Q, _lib.ptr(Kd), _lib.ptr(dd),
                                             _lib.ptr(out)), "spe_distort_points")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_against_ref(got, ref, what):
    p, s, st = got
    ulps = lr.ulp_diff(p, ref["points"]).max()
    print(what, "points: largest difference", ulps, "float32 ulp")
    assert (st == ref["status"]).all(), what
    assert ulps <= 1, what
    if s is not None:
        rel = (np.abs(s.astype(np.float64) - ref["sigmas64"]) / ref["sigmas64"]).max()
        print(what, "sigmas: largest relative difference", rel)
        assert rel <= 1e-5, what


@pytest.mark.parametrize("B,Q", [(1, 1), (3, 11), (1, 257), (7, 30)])
def test_kernel_matches_the_restatement(gpu_device, B, Q):
    """One point; one block's worth; one point past a 256-thread block (the bounds-checked tail);
    several images in one block."""
    rng = np.random.default_rng(1000 * B + Q)
    p = lr.random_points(rng, (B, Q))
    s = rng.uniform(0.5, 3.0, (B, Q, 2)).astype(np.float32)
    ref = lr.undistort_points(p, s)
    assert not ref["status"].any()
    assert np.abs(ref["points64"] - p).max() > (0.0 if Q == 1 else 5.0)        # the lens does move them
    got = _undistort(gpu_device, p, s)
    _check_against_ref(got, ref, f"B={B} Q={Q}")
    assert not got[2].any()
    # without sigmas: the same points, and nothing else is needed
    pn, sn, stn = _undistort(gpu_device, p)
    assert sn is None and pn.tobytes() == got[0].tobytes() and not stn.any()


def test_zero_distortion_copies_bit_for_bit(gpu_device):
    rng = np.random.default_rng(2)
    p = lr.random_points(rng, (3, 11))
    s = rng.uniform(1e-3, 3.0, (3, 11, 2)).astype(np.float32)
    p[0, 0] = (np.float32(0.1) + np.float32(959.9), np.float32(1e-30))          # (u - cx) / fx * fx + cx would round
    got = _undistort(gpu_device, p, s, scale=rng.uniform(50, 500, (3, 2)), dist=np.zeros(5))
    assert got[0].tobytes() == p.tobytes() and got[1].tobytes() == s.tobytes() and not got[2].any()


def test_in_place_equals_out_of_place(gpu_device):
    rng = np.random.default_rng(3)
    p = lr.random_points(rng, (3, 11))
    s = rng.uniform(0.5, 3.0, (3, 11, 2)).astype(np.float32)
    a = _undistort(gpu_device, p, s)
    b = _undistort(gpu_device, p, s, inplace=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (a[2] == b[2]).all()
    assert a[0].tobytes() != p.tobytes()


def test_null_scale_is_a_scale_of_ones(gpu_device):
    rng = np.random.default_rng(4)
    p = lr.random_points(rng, (3, 11))
    s = rng.uniform(0.5, 3.0, (3, 11, 2)).astype(np.float32)
    a = _undistort(gpu_device, p, s)
    b = _undistort(gpu_device, p, s, scale=np.ones((3, 2)))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_anisotropic_scale_matches_the_restatement(gpu_device):
    rng = np.random.default_rng(5)
    p = lr.random_points(rng, (3, 11))
    s = rng.uniform(0.5, 3.0, (3, 11, 2)).astype(np.float32)
    scale = np.tile(np.array([[2.0, 0.5]], np.float32), (3, 1))
    ref = lr.undistort_points(p, s, scale)
    _check_against_ref(_undistort(gpu_device, p, s, scale), ref, "scale (2, 0.5)")
    # and the scale matters: off the axes A12 mixes the two axes' pixel sigmas
    assert np.abs(ref["sigmas64"] / lr.undistort_points(p, s)["sigmas64"] - 1).max() > 1e-4


def test_bad_icd_returns_the_input_with_status_1(gpu_device):
    """dist = (-5, 0, 0, 0, 0): at r2 = 0.25 the radial factor is 1 - 1.25 < 0 in round 1.  The other
    points lie at r2 <= 0.02 (factor >= 0.9), inside the model's domain."""
    rng = np.random.default_rng(6)
    dist = np.array([-5.0, 0, 0, 0, 0])
    fx, fy, cx, cy = lr._k(K)
    xy = rng.uniform(-0.1, 0.1, (2, 7, 2))
    p = np.stack((cx + fx * xy[..., 0], cy + fy * xy[..., 1]), -1).astype(np.float32)
    good = p.copy()
    p[1, 3] = (cx + 0.5 * fx, cy)
    s = rng.uniform(0.5, 3.0, (2, 7, 2)).astype(np.float32)
    ref = lr.undistort_points(p, s, dist=dist)
    assert ref["status"].sum() == 1 and ref["status"][1, 3] == 1
    got = _undistort(gpu_device, p, s, dist=dist)
    _check_against_ref(got, ref, "bad icd")
    assert got[2][1, 3] == 1 and got[2].sum() == 1
    assert got[0][1, 3].tobytes() == p[1, 3].tobytes() and got[1][1, 3].tobytes() == s[1, 3].tobytes()
    # the other points are what they are without the bad one in the call
    alone = _undistort(gpu_device, good, s, dist=dist)
    keep = np.ones((2, 7), bool)
    keep[1, 3] = False
    assert got[0][keep].tobytes() == alone[0][keep].tobytes() and got[1][keep].tobytes() == alone[1][keep].tobytes()
    assert not alone[2].any()


def test_distort_then_undistort_returns_the_ideal_points(gpu_device):
    """The distorted point is rounded to float32: an error of up to half an ulp per coordinate, which
    A = D^-1 (|A11| <= 1.05, |A12| <= 0.015 here) carries into the ideal image as at most 0.54 ulp of the
    same coordinate plus 0.008 ulp of the other one (the 12-round residual, 1e-12 px, is nothing beside
    it).  The ideal point is a float32 itself, so the result rounds to within 1 ulp of it as long as the
    fp64 error stays below 1.5 of ITS ulp.  With every |coordinate| in [64, 2120] px the other coordinate's
    ulp is at most 32 times this one's (0.26 ulp), and with a shift of at most 31 px per axis the distorted
    coordinate lies in the same or a neighbouring binade (at most 2 * 0.54 ulp): 1.34 < 1.5.  So the
    points are drawn over the frame plus the margin outside the 64 px bands around the two zero lines.  The points as drawn, bands
    included, are checked too, in pixels, per axis: 0.54 ulp of the distorted coordinate (|A11| <= 1.05),
    0.008 ulp of the other distorted coordinate (|A12| <= 0.015) and half an ulp of the result."""
    rng = np.random.default_rng(7)
    p = lr.random_points(rng, (4, 64))
    p[0, :4] = [[3.5, -2.25], [-40.0, 600.0], [960.0, 0.5], [-0.125, 20.0]]       # inside the bands for certain
    drawn = p.copy()
    dd = _distort(gpu_device, drawn)
    bb, _, sb = _undistort(gpu_device, dd, iters=12)
    sp_d, sp_i = np.spacing(np.abs(dd)).astype(np.float64), np.spacing(np.abs(drawn)).astype(np.float64)
    tol = 0.54 * sp_d + 0.008 * sp_d[..., ::-1] + 0.5 * sp_i
    excess = (np.abs(bb.astype(np.float64) - drawn) / tol).max()
    print("distort -> undistort(12) on the points as drawn: largest error / bound", excess)
    assert not sb.any() and excess <= 1.0
    near0 = np.abs(p) < 64
    p[near0] = np.where(p[near0] < 0, p[near0] - 64, p[near0] + 64)
    d = _distort(gpu_device, p)
    ulps_d = lr.ulp_diff(d, lr.distort(p, K, DIST).astype(np.float32)).max()
    print("distort against the restatement:", ulps_d, "ulp; largest shift", np.abs(d - p).max(), "px")
    assert ulps_d <= 1
    back, _, st = _undistort(gpu_device, d, iters=12)
    ulps = lr.ulp_diff(back, p).max()
    print("distort -> undistort(12): largest difference", ulps, "float32 ulp")
    assert not st.any()
    assert ulps <= 1


# ------------------------------------------------------------------------------------------ wiring

def _rodrigues(r):
    th = np.linalg.norm(r)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _score64(rvec, tvec, q_gt, t_gt):
    """The SPEED score (REV/utils/speed_eval.py:245-262: rotation angle between the two attitudes +
    |t - t_gt| / |t_gt|) of the solver's fp64 pose.  The angle is taken from the relative rotation by
    atan2: 2 arccos(|<q, q_gt>|) on the solver's float32 quaternion cannot resolve angles below
    sqrt(2 * 2^-24) = 3.5e-4 rad (it returns 0 or about that), a thousand times the float32 pixel
    rounding this test measures, 1.2e-4 px / 3003 px = 4e-8 rad."""
    E = _rodrigues(rvec) @ quat_to_matrix(q_gt).T
    v = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / 2
    return np.arctan2(np.linalg.norm(v), (np.trace(E) - 1) / 2) + np.linalg.norm(tvec - t_gt) / np.linalg.norm(t_gt)


def _scene(B, seed, dist=None, noise=0.0):
    """B synthetic poses: the 11 landmarks projected (through the lens with dist), one query per
    landmark, float32 pixels."""
    from spe.synthetic import random_pose
    rng = np.random.default_rng(seed)
    q, t = random_pose(rng, B)
    W = world_points()
    pts = np.stack([project(W, q[i], t[i], dist=dist) for i in range(B)])
    pts = pts + rng.normal(0, noise, pts.shape) if noise else pts
    return q, t, pts.astype(np.float32)


def _one_hot(B, score=1.0):
    p = np.full((B, 11, 12), (1.0 - score) / 11, np.float32)
    p[:, np.arange(11), np.arange(11)] = score
    return p


def _clip(B, dev, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    xy = torch.rand(B, 2, generator=g) * 600
    wh = 200 + torch.rand(B, 2, generator=g) * 500          # non-square: the two axes scale differently
    return torch.cat([xy, xy + wh], 1).to(dev)


def _solvers(lens):
    from spe.solver import EPnPCeresSolver, EPnPSolver, ExhaustivePoseSolver, SimplePoseSolverSigma
    return {"epnp": EPnPSolver(lens=lens), "sigma": SimplePoseSolverSigma(lens=lens),
            "ceres": EPnPCeresSolver(lens=lens), "exhaustive": ExhaustivePoseSolver(lens=lens)}


@pytest.mark.parametrize("name", ["epnp", "sigma", "ceres", "exhaustive"])
def test_solver_with_a_lens_is_the_plain_solver_on_the_kernels_output(gpu_device, name):
    from spe.solver import sigma_scale_of
    dev, B = gpu_device, 4
    lens = LensModel(dist=DIST)
    _, _, pts = _scene(B, 21, dist=DIST, noise=0.7)
    rng = np.random.default_rng(22)
    clip = _clip(B, dev)
    scale = sigma_scale_of(clip, dev)
    points = torch.from_numpy(pts).to(dev)
    probs = torch.from_numpy(_one_hot(B, 0.89)).to(dev)
    sig = (torch.from_numpy(rng.uniform(0.5, 2.0, (B, 11, 2)).astype(np.float32)).to(dev) / scale[:, None, :]).contiguous()
    kw = {"area": [4000.0, 9000.0, 2500.0, 16000.0]} if name == "ceres" else {}
    with_lens, plain = _solvers(lens)[name], _solvers(None)[name]
    assert plain.lens is None and with_lens.lens is lens
    got = with_lens.solve_batch(points, probs, sig, sigma_scale=scale, **kw)
    torch.cuda.synchronize()
    assert got["lens_status"].dtype == torch.uint8 and not got["lens_status"].any()
    pi, si = got["points_ideal"].clone(), got["sigmas_ideal"].clone()
    # what the kernel gives on its own, and that it is not the input
    kp, ks, _ = _undistort(dev, pts, sig.cpu().numpy(), scale.cpu().numpy())
    assert pi.cpu().numpy().tobytes() == kp.tobytes() and si.cpu().numpy().tobytes() == ks.tobytes()
    assert (pi - points).abs().max() > 0.01
    ref = plain.solve_batch(pi, probs, si, **kw)
    assert "points_ideal" not in ref and "lens_status" not in ref
    for k in ("quat", "tvec", "rvec", "status", "inlier_mask"):
        assert torch.equal(got[k], ref[k]), (name, k)
    assert ((got["status"] == 0) | (got["status"] == 3)).all()
    # the covariance reads sigmas_ideal from the poses
    c_got = with_lens.pose_covariance(probs, sig, got, clip_bbox=clip)
    c_ref = plain.pose_covariance(probs, si, ref, clip_bbox=clip)
    for k in ("pose_cov", "sigma_rot", "sigma_t", "pred_score", "cov_status"):
        assert torch.equal(c_got[k], c_ref[k]), (name, k)
    assert (c_got["cov_status"] == 0).all()
    assert not torch.equal(c_got["pose_cov"], plain.pose_covariance(probs, sig, ref, clip_bbox=clip)["pose_cov"])


def test_end_to_end_lens_solver_recovers_the_ideal_camera_score(gpu_device):
    """8 synthetic poses, the landmarks seen through the lens.  Baseline: EPnP on the same poses projected
    without distortion, solved without a lens (the parent's behaviour on an ideal camera).  The lens
    solver must score within 10x of it on every image (float32 pixel rounding, 1.2e-4 px at 1920, against a
    3e-7 px iteration residual), and the plain solver on the distorted points worse than the lens solver
    on every image.  Scores: _score64.  Measured on an MI355X: see DESIGN."""
    from spe.solver import EPnPSolver
    dev, B = gpu_device, 8
    q, t, ideal = _scene(B, 0)
    _, _, seen = _scene(B, 0, dist=DIST)
    probs = torch.from_numpy(_one_hot(B)).to(dev)

    def scores(solver, pts):
        o = solver.solve_batch(torch.from_numpy(pts).to(dev), probs)
        torch.cuda.synchronize()
        assert (o["status"] == 0).all()
        rv, tv = o["rvec"].cpu().numpy(), o["tvec"].cpu().numpy()
        return np.array([_score64(rv[i], tv[i], q[i], t[i]) for i in range(B)])

    base = scores(EPnPSolver(), ideal)
    lens = scores(EPnPSolver(lens=LensModel(dist=DIST)), seen)
    none = scores(EPnPSolver(), seen)
    print("shift of the landmarks, px per image", np.abs(seen - ideal).max(axis=(1, 2)))
    for name, s in (("ideal camera, no lens", base), ("distorted, lens solver", lens), ("distorted, no lens", none)):
        print(f"score, {name}: {s.min():.3e} .. {s.max():.3e}")
    print("lens / baseline per image", lens / base)
    assert (lens <= 10 * base).all()
    assert (none > lens).all()
    # the shipped score path (spe_speed_score on the float32 quaternion): its angle comes in steps of about
    # 2 sqrt(2 * 2^-24) = 6.9e-4 rad near zero, so per image the lens solver's score may exceed the plain
    # solver's by no more than one such step (bound 1e-3), and over the batch it is the smaller one
    from spe.speed_eval import device_speed_score
    qd, td = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)

    def shipped(solver, pts):
        o = solver.solve_batch(torch.from_numpy(pts).to(dev), probs)
        s_t, s_q = device_speed_score(o["quat"], o["tvec"], qd, td)
        return (s_t + s_q).cpu().numpy()

    lens_dev, none_dev = shipped(EPnPSolver(lens=LensModel(dist=DIST)), seen), shipped(EPnPSolver(), seen)
    print("device score, lens solver", lens_dev, "no lens", none_dev)
    assert (lens_dev <= none_dev + 1e-3).all()
    assert lens_dev.sum() < none_dev.sum()


def test_sigma_ensemble_undistorts_every_model_in_one_launch(gpu_device):
    """M = 2 identical models through an ensemble with a lens: the fused arrays equal those of a lens-free
    ensemble fed the single-model undistortion, bit for bit.  Per-image crops of different, non-square
    sizes: a wrong [M * B, Q] layout of points, sigmas or scales would show."""
    from spe.solver import SigmaEnsemblePoseSolver, SimplePoseSolverSigma, sigma_scale_of
    dev, B = gpu_device, 3
    lens = LensModel(dist=DIST)
    _, _, pts = _scene(B, 31, dist=DIST, noise=0.5)
    rng = np.random.default_rng(32)
    clip = _clip(B, dev, 1)
    scale = sigma_scale_of(clip, dev)
    points = torch.from_numpy(pts).to(dev)
    probs = torch.from_numpy(_one_hot(B, 0.89)).to(dev)
    sig = (torch.from_numpy(rng.uniform(0.5, 2.0, (B, 11, 2)).astype(np.float32)).to(dev) / scale[:, None, :]).contiguous()
    ens = SigmaEnsemblePoseSolver(SimplePoseSolverSigma(), lens=lens)
    assert ens.lens is lens and ens.backend.lens is lens
    fused = ens.fuse_batch([points, points], [probs, probs], [sig, sig], clip_bbox=clip)
    torch.cuda.synchronize()
    assert fused["lens_status"].shape == (2, B, 11) and not fused["lens_status"].any()
    one = SimplePoseSolverSigma(lens=lens).undistort(points, sig, scale)
    pi, si = one["points_ideal"].clone(), one["sigmas_ideal"].clone()
    ref = SigmaEnsemblePoseSolver(SimplePoseSolverSigma()).fuse_batch([pi, pi], [probs, probs], [si, si], clip_bbox=clip)
    assert "lens_status" not in ref
    for k in ("points", "probs", "sigmas", "n_pooled", "n_kept"):
        assert torch.equal(fused[k], ref[k]), k
    assert (fused["n_kept"] == 2).all()
    # and the solve runs on the fused, already ideal arrays: no second undistortion
    poses = ens.solve_batch_multi([points, points], [probs, probs], [sig, sig], clip_bbox=clip)
    plain = SimplePoseSolverSigma().solve_batch(ref["points"], ref["probs"], ref["sigmas"])
    for k in ("quat", "tvec", "status", "inlier_mask"):
        assert torch.equal(poses[k], plain[k]), k
    assert "points_ideal" not in poses


def test_multi_mean_solver_undistorts_before_fusing(gpu_device):
    from spe.solver import Multi_Mean_PoseSolver
    dev, B = gpu_device, 3
    lens = LensModel(dist=DIST)
    _, _, pts = _scene(B, 41, dist=DIST, noise=0.5)
    points = torch.from_numpy(pts).to(dev)
    probs = torch.from_numpy(_one_hot(B, 0.89)).to(dev)
    other = points.flip(0).contiguous()
    fp, fr = Multi_Mean_PoseSolver(lens=lens).fuse_batch([points, other], [probs, probs])
    kp = [torch.from_numpy(_undistort(dev, p.cpu().numpy())[0]).to(dev) for p in (points, other)]
    rp, rr = Multi_Mean_PoseSolver().fuse_batch(kp, [probs, probs])
    assert torch.equal(fp, rp) and torch.equal(fr, rr)
    got = Multi_Mean_PoseSolver(lens=lens).solve_batch_multi([points, points], [probs, probs])
    ref = Multi_Mean_PoseSolver().solve_batch_multi([kp[0], kp[0]], [probs, probs])
    for k in ("quat", "tvec", "status"):
        assert torch.equal(got[k], ref[k]), k


def test_pose_pipeline_with_a_lens_in_every_eager_mode(gpu_device):
    """RT-DETR r18 at S = 128, B = 4 and a sigma solver with a lens: plain, overlap, overlap_decode,
    overlap_backbone and the two host_input modes.  Every mode returns lens_status all zero and the plain
    mode's poses, and the undistorted keypoints are the kernel's on that run's forward output with the
    crop's size as the sigma scale."""
    import argparse

    from spe.pipeline import PosePipeline
    from spe.solver import build_solver
    from test_gpu_rtdetr_stages import _clip as sq_clip, _crops, _model, _normalised
    dev, B, S = gpu_device, 4, 128
    m = _model("r18", "bf16")
    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma", dist=list(DIST)))
    assert solver.lens is not None
    crops = [_crops(B, S, 1, 40 + k, dev) for k in range(2)]
    images = [_normalised(c) for c in crops]
    clips = [sq_clip(B, dev, 10 + k) for k in range(2)]
    order = [0, 1, 0]

    def finish(p, outs):
        for o in outs:
            p.wait(o)
        torch.cuda.synchronize()
        for o in outs:
            assert o["poses"]["lens_status"].shape == (B, m.cfg.num_queries) and not o["poses"]["lens_status"].any()
        # the solver keeps one set of lens buffers per shape: they hold the last run's
        last, clip = outs[-1], clips[order[-1]]
        scale = torch.stack((clip[:, 2] - clip[:, 0], clip[:, 3] - clip[:, 1]), 1)
        kp, ks, _ = _undistort(dev, last["forward"]["points_px"].cpu().numpy(), last["forward"]["sigmas"].cpu().numpy(),
                               scale.cpu().numpy())
        assert last["poses"]["points_ideal"].cpu().numpy().tobytes() == kp.tobytes()
        assert last["poses"]["sigmas_ideal"].cpu().numpy().tobytes() == ks.tobytes()
        return [{k: o["poses"][k].clone() for k in ("status", "quat", "tvec")} for o in outs]

    def run_loaded(**kw):
        p = PosePipeline(m, solver, B, device=dev, pose_cov=True, **kw)
        outs = []
        for k in order:
            p.load(images[k], clips[k])
            outs.append(p.run())
        for o in outs:
            assert o["cov_status"].shape == (B,)
        return finish(p, outs)

    plain = run_loaded()
    modes = [("overlap", run_loaded(overlap=True)), ("overlap_decode", run_loaded(overlap_decode=True)),
             ("overlap_backbone", run_loaded(overlap_backbone=True))]
    for kw in (dict(overlap_backbone=True), {}):
        host = PosePipeline(m, solver, B, device=dev, host_input=True, **kw)
        host.load_host(torch.cat(crops).cpu(), torch.cat(clips).cpu(), torch.zeros(2 * B, 4, dtype=torch.float64),
                       torch.ones(2 * B, 3, dtype=torch.float64))
        modes.append((("host_input", tuple(kw)), finish(host, [host.run() for _ in order])))
    for what, outs in modes:
        for i, (o, r) in enumerate(zip(outs, plain)):
            for k in r:
                assert torch.equal(o[k], r[k]), (what, i, k)


def test_evaluate_rtdetr_hands_the_crop_scale_to_the_lens(gpu_device):
    """evaluate_rtdetr with a lens solver over two batches of a stand-in model that returns synthetic
    outputs seen through the lens, crop-normalised sigmas, non-square crops, off-centre satellites (so that
    A12 is ~1e-2 and the two axes' scales mix visibly): every record is the pose and the predicted score
    of solve_batch(..., sigma_scale=crop size) + pose_covariance done by hand, which a solve without the
    scale does not give."""
    import argparse

    from spe.engine import evaluate_rtdetr
    from spe.solver import build_solver, sigma_scale_of
    dev, B = gpu_device, 3
    W = world_points()
    rng = np.random.default_rng(51)
    names = [f"img{i}.jpg" for i in range(2 * B)]
    q = rng.normal(size=(2 * B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.stack([rng.uniform(1.2, 1.8, 2 * B), rng.uniform(-1.2, -0.8, 2 * B), rng.uniform(7, 10, 2 * B)], 1)
    gt = {n: {"quat": q[i].tolist(), "tvec": t[i].tolist()} for i, n in enumerate(names)}
    pts = np.stack([project(W, q[i], t[i], dist=DIST) for i in range(2 * B)]).astype(np.float32)
    clips = [_clip(B, dev, 20 + k) for k in range(2)]
    probs = torch.from_numpy(_one_hot(B, 0.89)).to(dev)
    sigs = [(torch.from_numpy(rng.uniform(0.5, 2.0, (B, 11, 2)).astype(np.float32)).to(dev)
             / sigma_scale_of(c, dev)[:, None, :]).contiguous() for c in clips]
    loader = [(torch.zeros(B, 3, 8, 8), [{"filename": names[k * B + b], "clip_bbox": clips[k][b].cpu()}
                                         for b in range(B)]) for k in range(2)]

    def model(samples, clip_bbox=None):
        k = [i for i in range(2) if torch.equal(clip_bbox, clips[i])][0]
        z = torch.zeros(B, 11, 12, device=dev)
        return {"points_px": torch.from_numpy(pts[k * B:(k + 1) * B]).to(dev), "probs": probs, "sigmas": sigs[k],
                "pred_logits": z, "aux_outputs": [{"pred_logits": z} for _ in range(3)]}

    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma", dist=list(DIST)))
    _, ev = evaluate_rtdetr(model, None, None, loader, gt, solver, dev, pose_cov=True)
    differs = 0
    for k in range(2):
        p = torch.from_numpy(pts[k * B:(k + 1) * B]).to(dev)
        poses = solver.solve_batch(p, probs, sigs[k], sigma_scale=sigma_scale_of(clips[k], dev))
        cov = solver.pose_covariance(probs, sigs[k], poses, clip_bbox=clips[k])
        si = poses["sigmas_ideal"].clone()
        unscaled = solver.solve_batch(p, probs, sigs[k])
        assert not torch.equal(unscaled["sigmas_ideal"], si)
        cov_u = solver.pose_covariance(probs, sigs[k], unscaled, clip_bbox=clips[k])
        assert (cov["cov_status"] == 0).all()
        ps, ps_u = cov["pred_score"].cpu().numpy(), cov_u["pred_score"].cpu().numpy()      # float32, as logged
        for b in range(B):
            rec = ev.log[names[k * B + b]]
            assert rec["quat_pr"] == np.around(poses["quat"][b].double().cpu().numpy(), decimals=6).tolist()
            assert rec["tvec_pr"] == np.around(poses["tvec"][b].cpu().numpy(), decimals=6).tolist()
            assert rec["cov_status"] == 0
            assert rec["pred_score"] == float(np.around(ps[b], decimals=8))
            assert rec["score"] < 1e-3                      # through the lens the pose is the true one
            differs += rec["pred_score"] != float(np.around(ps_u[b], decimals=8))
    assert differs > 0
