"""GPU: spe_calibration_records (csrc/calib.hip) against tests/calibration_ref.py on poses and covariances
the device itself produced from synthetic keypoints, one batch with every status and flag case, determinism,
the argument refusals, the statistical loop through spe.calibration.Calibration, evaluate_rtdetr and the
staged PosePipeline.  No model output is used: the keypoints are synthetic, as in
tests/test_gpu_pose_covariance.py, whose helpers (and solved cases) this file shares.

Tolerances, both sides fp64:
  delta (rotation)  the kernel multiplies two unit quaternions (rvec's, from one sincos, and q_gt's conjugate:
                    4 products and 3 sums per component, <= 8 eps) and takes one atan2; the reference multiplies
                    two rotation matrices (entries <= ~8 eps each, the product <= ~30 eps) and reads the
                    quaternion off it (<= ~20 eps).  Both errors are absolute, on quantities of size <= 1, and the
                    angle doubles them: 2 (8 + 30 + 20) eps, rounded up to 128 eps max(1, |dw|).
  delta (transl.)   one subtraction of the same fp64 inputs: exact on both sides, 2 eps |t| allowed.
  z                 the projection is ~12 operations on camera coordinates, then fx x / z + cx of size |u| <=
                    ~2e3 px: <= 16 eps (|p| + |u|) absolute in the numerator on either side, over the effective sigma,
                    plus 4 eps |z| for the sigma product and the division:  (32 eps (|p| + |u|)) / sigma + 8 eps |z|.
  nees              64 eps kappa nees, kappa the condition number of the scaled matrix, the form
                    tests/test_gpu_pose_covariance.py uses for the covariance.  The reference value is the
                    reference's solve (calibration_ref.nees_of) of the same matrix applied to the DEVICE's delta, so
                    the bound measures the solve alone: delta has its own check above, and its allowed error
                    carried through the quadratic form would exceed this bound by orders of magnitude.
kp_flags and calib_status are compared exactly.  The largest observed ratio to each bound is printed.
"""
import argparse

import numpy as np
import pytest

import calibration_ref as cr
import pose_covariance_ref as pc
import postmodel_ref as pr
import test_gpu_pose_covariance as tpc

pytestmark = pytest.mark.gpu

SPE_E_ARG = -1
FILL = -7
EPS = np.finfo(np.float64).eps
OUT = ("delta", "nees", "z", "kp_flags", "calib_status")
_dev = tpc._dev


def call_records(dev, x, scale=None, floor=1e-3, gain=1.0, B=None, Q=None, C=None):
    """spe_calibration_records through ctypes on numpy inputs (x: the reference's keyword arguments); the
    outputs start filled with a sentinel.  -> rc, dict of device tensors."""
    import torch
    from spe import _lib
    b, q, c = x["probs"].shape
    L = c - 1
    out = dict(delta=torch.full((b, 6), FILL, dtype=torch.float64, device=dev),
               nees=torch.full((b, 3), FILL, dtype=torch.float64, device=dev),
               z=torch.full((b, L, 2), FILL, dtype=torch.float64, device=dev),
               kp_flags=torch.full((b, L), 249, dtype=torch.uint8, device=dev),
               calib_status=torch.full((b,), FILL, dtype=torch.int32, device=dev))
    f32, f64, i32 = np.float32, np.float64, np.int32
    ins = [_dev(np.asarray(x["points"], f32), dev), _dev(np.asarray(x["probs"], f32), dev),
           _dev(np.asarray(x["sigmas"], f32), dev), _dev(scale, dev)]
    mid = [_dev(np.asarray(x["status"], i32), dev), _dev(np.asarray(x["corr_label"], i32), dev),
           _dev(np.asarray(x["inlier_mask"], np.uint32).view(i32), dev), _dev(np.asarray(x["rvec"], f64), dev),
           _dev(np.asarray(x["tvec"], f64), dev), _dev(np.asarray(x["q_gt"], f64), dev),
           _dev(np.asarray(x["t_gt"], f64), dev), _dev(np.asarray(x["cov"], f64), dev),
           _dev(np.asarray(x["cov_status"], i32), dev)]
    K, W = _dev(np.asarray(x["K"], f64), dev), _dev(np.asarray(x["world"], f64), dev)
    rc = _lib.lib().spe_calibration_records(
        _lib.stream_ptr(), *[_lib.ptr(a) for a in ins], floor, *[_lib.ptr(a) for a in mid], b if B is None else B,
        q if Q is None else Q, c if C is None else C, _lib.ptr(K), _lib.ptr(W), gain, *[_lib.ptr(out[k]) for k in OUT])
    torch.cuda.synchronize()
    return rc, out


def _untouched(out):
    return all(bool((t == (249 if k == "kp_flags" else FILL)).all()) for k, t in out.items())


def to_numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_records(got, ref, x, scale, floor, gain, what):
    """Device records (numpy) against the reference's; -> the largest error / bound per output."""
    np.testing.assert_array_equal(got["calib_status"], ref["calib_status"], err_msg=str(what))
    np.testing.assert_array_equal(got["kp_flags"], ref["kp_flags"], err_msg=str(what))
    for k in ("delta", "nees", "z"):
        assert np.isfinite(got[k]).all(), (what, k)
    st = ref["calib_status"]
    assert not got["delta"][(st == 1) | (st == 2)].any() and not got["nees"][st != 0].any()
    assert not got["z"][(ref["kp_flags"] & 1) == 0].any()
    worst = dict(delta=0.0, z=0.0, nees=0.0)
    B, Q, C = x["probs"].shape
    K = np.asarray(x["K"], np.float64)
    for b in range(B):
        d, r = got["delta"][b], ref["delta"][b]
        bw = 128 * EPS * max(1.0, np.linalg.norm(r[:3]))
        bt = 2 * EPS * max(np.abs(x["tvec"][b]).max(), np.abs(x["t_gt"][b]).max()) + 1e-300
        worst["delta"] = max(worst["delta"], np.abs(d[:3] - r[:3]).max() / bw, np.abs(d[3:] - r[3:]).max() / bt)
        assert np.abs(d[:3] - r[:3]).max() <= bw and np.abs(d[3:] - r[3:]).max() <= bt, (what, b, d - r)
        if st[b] == 1:
            continue
        labs, sel_p = cr.pnp_ref.select_correspondences(np.asarray(x["points"][b], np.float32), x["probs"][b])
        _, sel_s = cr.pnp_ref.select_correspondences(np.asarray(x["sigmas"][b], np.float32), x["probs"][b])
        sc = np.ones(2) if scale is None else scale[b].astype(np.float64)
        for i, l in enumerate(labs):
            if not ref["kp_flags"][b, l] & 1:
                continue
            sg = np.maximum(sel_s[i].astype(np.float64) * sc * gain, np.float64(np.float32(floor)))
            p = np.abs(sel_p[i].astype(np.float64))
            bound = 32 * EPS * (p + np.abs(p - ref["z"][b, l] * sg)) / sg + 8 * EPS * np.abs(ref["z"][b, l])
            err = np.abs(got["z"][b, l] - ref["z"][b, l])
            worst["z"] = max(worst["z"], (err / bound).max())
            assert (err <= bound).all(), (what, b, l, err, bound)
        if st[b] == 0:
            S = np.asarray(x["cov"][b], np.float64) * (gain * gain)
            for j, (blk, dd) in enumerate(((S, d), (S[:3, :3], d[:3]), (S[3:, 3:], d[3:]))):
                v, kappa = cr.nees_of(blk, dd)                 # the reference's solve on the device's own delta
                assert v is not None and kappa <= 1e10, (what, b, j, kappa)
                bound = 64 * EPS * kappa * v
                err = abs(got["nees"][b, j] - v)
                worst["nees"] = max(worst["nees"], err / bound)
                assert err <= bound, (what, b, j, err, bound, kappa)
    print(what, "largest error / bound:", {k: "%.3g" % v for k, v in worst.items()})
    return worst


def quats_of(R):
    return np.stack([cr.pnp_ref.blender_quat(r).astype(np.float64) for r in R])


def solved_case(dev, B, Q, C, scale=None):
    """The pose-covariance test's solved case plus the device's own covariance and a ground truth: the true
    poses of the keypoint set."""
    import torch
    from spe.config import Camera
    pts, probs, sig, _ = tpc.inputs(B, Q, C)
    _, _, _, R, t = pc.keypoint_set(B, Q, C, pr.world_for(C), Camera.K, seed=1000 * B + 10 * Q + C)
    h = tpc.solved(B, Q, C)
    rc, cov = tpc.call_cov(dev, probs, sig, h["status"], h["corr_label"], h["solver_mask"], h["rvec"], h["tvec"], C, scale)
    assert rc == 0
    return dict(points=pts, probs=probs, sigmas=sig, status=h["status"], corr_label=h["corr_label"],
                inlier_mask=h["solver_mask"], rvec=h["rvec"], tvec=h["tvec"], q_gt=quats_of(R), t_gt=t,
                cov=cov["cov"].cpu().numpy(), cov_status=cov["cov_status"].cpu().numpy(), K=Camera.K, world=pr.world_for(C))


# B = 5 does not fill a work-group of four images; Q = 64, C = 17 are the limits
@pytest.mark.parametrize("B,Q,C,scaled,gain", [(5, 11, 12, False, 1.0), (5, 30, 12, True, 1.0), (1, 64, 17, True, 1.75)])
def test_kernel_matches_reference(gpu_device, B, Q, C, scaled, gain):
    scale = tpc.inputs(B, Q, C)[3] if scaled else None
    x = solved_case(gpu_device, B, Q, C, scale)
    rc, out = call_records(gpu_device, x, scale=scale, gain=gain)
    assert rc == 0
    ref = cr.calibration_records(**x, sigma_scale=scale, sigma_gain=gain)
    assert (ref["calib_status"] == 0).all()                 # every image solved, with a covariance
    check_records(to_numpy(out), ref, x, scale, 1e-3, gain, (B, Q, C))
    # |dw| is the score's rotation angle a, up to the float32 quaternion the score reads.  Its dot product d = cos(a / 2)
    # carries dd <= 8 * 2^-24 (four products of float32-rounded components, and the two quaternions' norms, which the
    # score does not divide by, are 1 to 2^-23 each).  Near d = 1 the arccos is not linear: 1 - d = a^2 / 8, so the score
    # reads sqrt(a^2 -+ 8 dd) (0 once d is clipped at 1), at most a - sqrt(max(a^2 - 8 dd, 0)) away.
    import torch
    from spe.speed_eval import device_speed_score
    h = tpc.solved(B, Q, C)
    s_t, s_q = device_speed_score(_dev(h["quat"], gpu_device), _dev(h["tvec"], gpu_device), _dev(x["q_gt"], gpu_device),
                                  _dev(x["t_gt"], gpu_device))
    torch.cuda.synchronize()
    ang = np.linalg.norm(out["delta"].cpu().numpy()[:, :3], axis=1)
    dd = 8 * 2.0 ** -24
    assert (np.abs(ang - s_q.cpu().numpy()) <= ang - np.sqrt(np.maximum(ang * ang - 8 * dd, 0)) + 2.0 ** -40).all()


def mixed_case(dev):
    """12 images of the statistical experiment's kind, solved on the device, doctored into every case."""
    import torch
    from spe.config import Camera
    from spe.solver import SimplePoseSolverSigma
    pts, probs, sig, q_gt, t_gt, _ = cr.experiment_inputs(12, seed=99)
    probs[5, 0] = 0.01
    probs[5, 0, 11] = 0.8                                    # image 5: its first query is background, a landmark nobody carries
    solver = SimplePoseSolverSigma()
    d = [_dev(a, dev) for a in (pts, probs, sig)]
    poses = solver.solve_batch(*d)
    torch.cuda.synchronize()
    h = {k: poses[k].cpu().numpy() for k in ("status", "corr_label", "inlier_mask", "rvec", "tvec")}
    assert (h["status"] == 0).all()
    mask = h["inlier_mask"].view(np.uint32).copy()
    sig = sig.copy()
    for b in (7, 8):                                         # a NaN sigma on the query of correspondence 0 ...
        l = int(h["corr_label"][b, 0])
        sig[b, int(np.nonzero(probs[b].argmax(1) == l)[0][0]), 1] = np.nan
    mask[7] &= ~np.uint32(1)                                 # ... which in image 7 is no inlier, in image 8 is one
    assert mask[8] & 1
    h["status"][1] = 2                                       # no pose
    rc, cov = tpc.call_cov(dev, probs, sig, h["status"], h["corr_label"], mask, h["rvec"], h["tvec"], 12)
    assert rc == 0
    cov, cs = cov["cov"].cpu().numpy(), cov["cov_status"].cpu().numpy()
    assert cs[1] == 1 and cs[8] == 3 and cs[7] == 0
    for b, s in ((2, 2), (3, 3), (4, 4)):                    # the covariance's other refusals
        cs[b] = s
        cov[b] = 0
    cov[9] = 0                                               # a covariance of zeros that claims to be one: singular
    q_gt[0] = 0                                              # unusable ground truth
    t_gt[6] = [0.0, 0.0, 0.0]                                # the body's origin in the camera: landmarks on both sides
    want = np.array([1, 2, 3, 3, 3, 0, 0, 0, 3, 4, 0, 0], np.int32)
    return dict(points=pts, probs=probs, sigmas=sig, status=h["status"], corr_label=h["corr_label"], inlier_mask=mask,
                rvec=h["rvec"], tvec=h["tvec"], q_gt=q_gt, t_gt=t_gt, cov=cov, cov_status=cs, K=Camera.K,
                world=pr.world_for(12)), want


def test_every_status_and_flag_in_one_batch(gpu_device):
    x, want = mixed_case(gpu_device)
    scale = np.random.default_rng(4).uniform(0.5, 4.0, (12, 2)).astype(np.float32)
    for sc, gain in ((None, 1.0), (scale, 2.5)):
        rc, out = call_records(gpu_device, x, scale=sc, gain=gain)
        assert rc == 0
        got = to_numpy(out)
        ref = cr.calibration_records(**x, sigma_scale=sc, sigma_gain=gain)
        np.testing.assert_array_equal(ref["calib_status"], want)
        check_records(got, ref, x, sc, 1e-3, gain, ("mixed", gain))
        f = got["kp_flags"]
        assert not f[0].any() and (f[1] == 1).all()                      # no ground truth: nothing; no pose: no inliers
        assert (f[5] == 0).sum() == 1 and set(f[6]) <= {2, 3} and 0 < (f[6] & 1).sum() < 11
        l7, l8 = int(x["corr_label"][7, 0]), int(x["corr_label"][8, 0])
        assert f[7, l7] == 0 and f[8, l8] == 2                             # NaN sigma: never valid; inlier bit as the mask says
        assert set(got["calib_status"]) == {0, 1, 2, 3, 4}


def test_two_runs_give_the_same_bits(gpu_device):
    import torch
    x = solved_case(gpu_device, 5, 30, 12)
    runs = [call_records(gpu_device, x, gain=1.3) for _ in range(2)]
    assert runs[0][0] == 0 and runs[1][0] == 0
    for k in OUT:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


@pytest.mark.parametrize("case", ["q65", "c1", "c18", "b0", "gain0", "gain_nan", "gain_inf"])
def test_refusals_leave_the_outputs_alone(gpu_device, case):
    from spe import _lib
    x = solved_case(gpu_device, 5, 30, 12)
    kw = dict(q65=dict(Q=65), c1=dict(C=1), c18=dict(C=18), b0=dict(B=0), gain0=dict(gain=0.0),
              gain_nan=dict(gain=float("nan")), gain_inf=dict(gain=float("inf")))[case]
    rc, out = call_records(gpu_device, x, **kw)
    assert rc == SPE_E_ARG and _lib.lib().spe_last_error()
    assert _untouched(out)


# ---------------------------------------------------------------- the Python layer
def _compare(a, b, path="", scale=1.0):
    """Summary dicts: integers exactly, floats to 1e-12 relative (a mean of signed values relative to the mean
    magnitude beside it)."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _compare(a[k], b[k], f"{path}.{k}", a.get("mean_abs_z", 1.0) if k == "mean_z" else 1.0)
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _compare(u, v, f"{path}[{i}]", scale)
    elif isinstance(a, int):
        assert a == b, (path, a, b)
    else:
        assert abs(a - b) <= 1e-12 * max(abs(b), scale if "mean_z" in path else 0.0), (path, a, b)


def _loop(dev, data, gain, solver):
    """8 batches of 64 through the sigma solver, pose_covariance, the score and Calibration.update."""
    import torch
    from spe.calibration import Calibration
    from spe.speed_eval import device_speed_score
    pts, probs, sig, q_gt, t_gt, _ = data
    cal = Calibration(sigma_gain=gain, solver=solver)
    for k in range(8):
        s = slice(64 * k, 64 * k + 64)
        d = [_dev(a[s], dev) for a in (pts, probs, sig, q_gt, t_gt)]
        poses = solver.solve_batch(d[0], d[1], d[2])
        cov = solver.pose_covariance(d[1], d[2], poses)
        s_t, s_q = device_speed_score(poses["quat"], poses["tvec"], d[3], d[4])
        cal.update(d[0], d[1], d[2], poses, cov, d[3], d[4], s_t, s_q)
    summary = cal.summarize()
    rec = {k: v.cpu().numpy() for k, v in cal.records().items()}
    ref = cr.summarize(rec, rec["score"], rec["pred_score"], rec["cov_status"], sigma_gain=gain)
    _compare(summary, ref)
    assert (rec["calib_status"] == 0).all() and (rec["kp_flags"] == 3).all()      # the gates' condition
    t, frac = cal.threshold_for(float(np.median(rec["score"])))
    assert (t, frac) == cr.threshold_for(rec["pred_score"], rec["score"], float(np.median(rec["score"])))
    return summary


def test_statistical_loop_on_the_device(gpu_device):
    """The CPU test's gates on 512 images solved by the device's sigma solver: the reported sigma_gain within its
    gate of 2 at gain 1; with that gain fed back, the mean NEES and the coverage within theirs.  The sigmas are
    equal inside an image (calibration_ref.experiment_inputs says why)."""
    from spe.solver import SimplePoseSolverSigma
    data = cr.experiment_inputs(512, per_image_sigma=True)
    solver = SimplePoseSolverSigma()
    gate = cr.gates(512)
    s1 = _loop(gpu_device, data, 1.0, solver)
    g = s1["sigma_gain"]
    print("sigma_gain", g, gate["sigma_gain"], "mean NEES at gain 1", s1["pose"]["mean_nees"])
    assert gate["sigma_gain"][0] <= g <= gate["sigma_gain"][1]
    s2 = _loop(gpu_device, data, g, solver)
    print("fed back: mean NEES", s2["pose"]["mean_nees"], gate["mean_nees"], "coverage", s2["keypoints"]["inliers"]["coverage"],
          gate["coverage"], "AUSE", s2["sparsification"]["ause"], "Spearman", s2["sparsification"]["spearman"])
    assert gate["mean_nees"][0] <= s2["pose"]["mean_nees"][0] <= gate["mean_nees"][1]
    for c, (lo, hi) in zip(s2["keypoints"]["inliers"]["coverage"], gate["coverage"]):
        assert lo <= c <= hi
    assert s2["gain_in_force"] == g and abs(s2["sigma_gain"] - g) <= 1e-9 * g


def test_unequal_sigmas_through_the_sigma_solver_are_reported(gpu_device):
    """The same loop with sigmas drawn per keypoint and axis, the case a calibration is there to expose.  The
    keypoint side does not depend on the solver, so sigma_gain keeps its gate.  The pose side is REPORTED, not
    gated: the sigma solver's LM weighs a residual by 1 / sqrt(sigma) (the reference's rule), not by the 1 / sigma
    the covariance assumes, so its poses scatter more than the first-order covariance says.  Measured on an MI355X
    with the gain (2.0135) fed back: mean NEES 6.593 / 3.241 / 3.253 (full, rotation, translation) against 5.999 /
    2.957 / 2.970 with equal sigmas, cov_gain 2.111, shares below the chi-square 50 / 90 / 99 % quantiles 0.436 / 0.865 /
    0.984, AUSE 0.125, Spearman 0.62."""
    from spe.solver import SimplePoseSolverSigma
    data = cr.experiment_inputs(512, per_image_sigma=False)
    solver = SimplePoseSolverSigma()
    gate = cr.gates(512)
    s1 = _loop(gpu_device, data, 1.0, solver)
    g = s1["sigma_gain"]
    assert gate["sigma_gain"][0] <= g <= gate["sigma_gain"][1]
    s2 = _loop(gpu_device, data, g, solver)
    for c, (lo, hi) in zip(s2["keypoints"]["inliers"]["coverage"], gate["coverage"]):
        assert lo <= c <= hi
    print("unequal sigmas: sigma_gain", g, "fed back: mean NEES", s2["pose"]["mean_nees"], "cov_gain", s2["pose"]["cov_gain"],
          "shares below chi2", s2["pose"]["below_chi2"]["full"]["share"], "AUSE", s2["sparsification"]["ause"],
          "Spearman", s2["sparsification"]["spearman"])
    assert s2["pose"]["count"] == 512 and np.isfinite(s2["pose"]["mean_nees"]).all()


def test_evaluate_appends_the_calibration(gpu_device):
    """evaluate(calibration=True) over two batches of a stand-in model with a sigma head: the summary is under
    "calibration", the log and the stats' prefix are those of a run without it, and the summary is the one a
    Calibration fed by hand with the same batches gives."""
    import torch
    from spe.calibration import Calibration
    from spe.engine import evaluate
    from spe.solver import build_solver
    from spe.speed_eval import device_speed_score
    dev, B, Q = gpu_device, 3, 30
    names = [f"img{i}.jpg" for i in range(2 * B)]
    gt = {n: {"quat": [1.0, 0.0, 0.0, 0.0], "tvec": [0.0, 0.0, 8.0]} for n in names}
    clips = [tpc._boxes(B, 60 + k) for k in range(2)]
    synth = [tpc._synthetic_outputs(B, Q, 50 + k, clips[k]) for k in range(2)]
    loader = [(torch.zeros(B, 3, 8, 8), [{"filename": names[k * B + b], "clip_bbox": torch.from_numpy(clips[k][b])}
                                         for b in range(B)]) for k in range(2)]

    def model(samples, clip_bbox=None):
        k = [i for i in range(2) if np.array_equal(clip_bbox.cpu().numpy(), clips[i])][0]
        pts, probs, sig = [_dev(a, dev) for a in synth[k]]
        return {"points_px": pts, "probs": probs, "sigmas": sig}

    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma"))
    sp, ep = evaluate(model, None, None, loader, gt, solver, dev)
    sc, ec = evaluate(model, None, None, loader, gt, solver, dev, calibration=True, sigma_gain=1.5)
    assert "calibration" not in sp and ec.log == ep.log
    assert ec.stats.startswith(ep.stats) and "calibration: sigma gain" in ec.stats[len(ep.stats):]
    assert sc["speed_eval_pose"] == ec.stats
    cal = Calibration(sigma_gain=1.5, solver=solver)
    q_gt = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * B, dtype=torch.float64, device=dev)
    t_gt = torch.tensor([[0.0, 0.0, 8.0]] * B, dtype=torch.float64, device=dev)
    for k in range(2):
        d = [_dev(a, dev) for a in synth[k]]
        clip = _dev(clips[k], dev)
        poses = solver.solve_batch(*d)
        s_t, s_q = device_speed_score(poses["quat"], poses["tvec"], q_gt, t_gt)
        cal.update(d[0], d[1], d[2], poses, solver.pose_covariance(d[1], d[2], poses, clip_bbox=clip), q_gt, t_gt, s_t, s_q,
                   clip_bbox=clip)
    assert sc["calibration"] == cal.summarize()
    assert sc["calibration"]["gain_in_force"] == 1.5 and sc["calibration"]["pose"]["count"] == 2 * B
    # a model without a sigma head is refused
    with pytest.raises(ValueError, match="sigma head"):
        evaluate(lambda s, clip_bbox=None: {k: v for k, v in model(s, clip_bbox).items() if k != "sigmas"}, None, None,
                 loader, gt, build_solver(argparse.Namespace(solver="ransac_p3p_lm")), dev, calibration=True)


def test_evaluate_rtdetr_appends_the_calibration(gpu_device):
    """evaluate_rtdetr(calibration=True) with the stand-in model of the pose-covariance tests: the summary is
    there, the log entries and the stats' prefix are those of a run without it, and sigma_gain=1.0 changes
    no bit of a pose_cov run."""
    import torch
    from spe.engine import evaluate_rtdetr
    from spe.solver import build_solver
    dev, B, Q = gpu_device, 3, 30
    names = [f"img{i}.jpg" for i in range(2 * B)]
    gt = {n: {"quat": [1.0, 0.0, 0.0, 0.0], "tvec": [0.0, 0.0, 8.0]} for n in names}
    clips = [tpc._boxes(B, 60 + k) for k in range(2)]
    synth = [tpc._synthetic_outputs(B, Q, 50 + k, clips[k]) for k in range(2)]
    loader = [(torch.zeros(B, 3, 8, 8), [{"filename": names[k * B + b], "clip_bbox": torch.from_numpy(clips[k][b])}
                                         for b in range(B)]) for k in range(2)]

    def model(samples, clip_bbox=None):
        k = [i for i in range(2) if np.array_equal(clip_bbox.cpu().numpy(), clips[i])][0]
        pts, probs, sig = [_dev(a, dev) for a in synth[k]]
        z = torch.zeros(B, Q, 12, device=dev)
        return {"points_px": pts, "probs": probs, "sigmas": sig, "pred_logits": z,
                "aux_outputs": [{"pred_logits": z} for _ in range(3)]}

    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma"))
    runs = {}
    for name, kw in (("plain", {}), ("cal", dict(calibration=True)), ("cov", dict(pose_cov=True)),
                     ("cov_gain1", dict(pose_cov=True, sigma_gain=1.0)), ("cov_gain2", dict(pose_cov=True, sigma_gain=2.0)),
                     ("cov_cal", dict(pose_cov=True, calibration=True, sigma_gain=2.0))):
        runs[name] = evaluate_rtdetr(model, None, None, loader, gt, solver, dev, **kw)
    (sp, ep), (sc, ec) = runs["plain"], runs["cal"]
    assert "calibration" not in sp and ec.log == ep.log
    assert ec.stats.startswith(ep.stats) and "calibration: sigma gain" in ec.stats[len(ep.stats):]
    assert sc["speed_eval_pose"] == ec.stats and {k: v for k, v in sc.items() if k not in ("calibration", "speed_eval_pose")} == \
        {k: v for k, v in sp.items() if k != "speed_eval_pose"}
    cal = sc["calibration"]
    assert cal["pose"]["count"] == 2 * B and cal["sparsification"]["count"] == 2 * B
    assert cal["keypoints"]["inliers"]["count"] > 0 and cal["gain_in_force"] == 1.0
    assert runs["cov_gain1"][1].log == runs["cov"][1].log
    a, b = runs["cov"][1].log, runs["cov_gain2"][1].log
    for n in names:                                          # the gain scales the predicted score, and nothing else
        assert abs(b[n]["pred_score"] - 2 * a[n]["pred_score"]) <= 2e-8 + 2.0 ** -21 * a[n]["pred_score"]
        assert {k: v for k, v in a[n].items() if k != "pred_score"} == {k: v for k, v in b[n].items() if k != "pred_score"}
    assert runs["cov_cal"][1].log == b and runs["cov_cal"][0]["calibration"]["gain_in_force"] == 2.0


def test_staged_pipeline_records_use_each_batch_s_boxes(gpu_device):
    """PosePipeline(calibration=..., overlap_backbone=True) on a small RT-DETR whose outputs are overwritten
    with synthetic keypoints: two batches with different crop boxes and ground truths in flight, each batch's
    records are the reference's for its own boxes (the sigmas are crop-normalised: another batch's boxes
    would move every z-score)."""
    import torch
    from spe.calibration import Calibration
    from spe.config import Camera
    from spe.pipeline import PosePipeline
    from spe.rtdetr import RTDETR
    from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights
    from spe.solver import build_solver
    dev, B, S = gpu_device, 3, 128
    cfg = RtdetrConfig(depth=18, input_size=S)
    real = RTDETR(cfg, dtype="bf16")
    real.load_state_dict(random_rtdetr_weights(cfg, 0))
    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma"))
    images = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(5)).to(dev)
    clips = [tpc._boxes(B, 70 + k) for k in range(2)]
    synth = [tpc._synthetic_outputs(B, cfg.num_queries, 80 + k, clips[k]) for k in range(2)]
    truth = [pc.keypoint_set(B, cfg.num_queries, 12, pr.world_for(12), Camera.K, seed=80 + k)[3:] for k in range(2)]
    dclips = [_dev(c, dev) for c in clips]
    m = tpc._Doctored(real, list(zip(dclips, synth)), dev)
    cal = Calibration(sigma_gain=1.5, solver=solver)
    p = PosePipeline(m, solver, B, device=dev, overlap_backbone=True, calibration=cal)
    res = []
    for k in range(2):
        p.load(images, dclips[k], _dev(quats_of(truth[k][0]), dev), _dev(truth[k][1], dev))
        res.append(p.run())
    for o in res:
        p.wait(o)
    torch.cuda.synchronize()
    for k, o in enumerate(res):
        assert (o["poses"]["status"] == 0).all() and (o["cov_status"] == 0).all()
        h = {n: o["poses"][n].cpu().numpy() for n in ("status", "corr_label", "inlier_mask", "rvec", "tvec")}
        x = dict(points=synth[k][0], probs=synth[k][1], sigmas=synth[k][2], status=h["status"], corr_label=h["corr_label"],
                 inlier_mask=h["inlier_mask"].view(np.uint32), rvec=h["rvec"], tvec=h["tvec"], q_gt=quats_of(truth[k][0]),
                 t_gt=truth[k][1], cov=o["pose_cov"].cpu().numpy(), cov_status=o["cov_status"].cpu().numpy(), K=Camera.K,
                 world=pr.world_for(12))
        scale = tpc._scale_of(clips[k])
        ref = cr.calibration_records(**x, sigma_scale=scale, sigma_gain=1.5)
        got = {n: o["calibration"][n].cpu().numpy() for n in OUT}
        check_records(got, ref, x, scale, 1e-3, 1.5, ("pipeline", k))
        other = cr.calibration_records(**x, sigma_scale=tpc._scale_of(clips[1 - k]), sigma_gain=1.5)
        assert np.abs(other["z"] - ref["z"]).max() > 1e-3
    s = cal.summarize()
    assert s["pose"]["count"] == 2 * B and s["gain_in_force"] == 1.5
