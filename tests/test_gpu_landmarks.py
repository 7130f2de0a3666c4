"""GPU: spe_landmarks_solve and spe_landmark_observations (csrc/landmarks.hip) against tests/landmarks_ref.py
at the smallest shapes that can break them, determinism, the selection, and the Python layer end to end
(evaluate_rtdetr(landmarks=rec) on a stand-in model, spe.landmarks, the solvers' world=).

Tolerance.  Statuses, n_used and obs_flags are compared exactly.  world, cov, chi2 and rms_px are sums over
views followed by ill-conditioned 3x3 solves, so their rounding error is measured, not chosen: the restatement
runs twice, with the views in forward and in reversed order, and the bound of each output is 16 x the largest
difference between the two runs, with a floor of 1e-12 of the output's largest magnitude.  The kernel's order
(a butterfly per wave, then lane-strided partials) is a third one; the factor covers it.  Both the spread and
the kernel's error are printed per case.
"""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest

import landmarks_ref as lr
from conftest import GOLDEN
from spe.config import Camera, world_points

pytestmark = pytest.mark.gpu

K = np.asarray(Camera.K, np.float64)
W = world_points()
W16 = np.concatenate([W, np.random.default_rng(5).uniform(-0.6, 0.6, (5, 3))])
NUM = ("world", "cov", "chi2", "rms_px")


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def fixture_case():
    with open(os.path.join(GOLDEN, "pnp_kat_wz_real.json")) as f:
        im = json.load(f)["images"]
    return dict(q=np.array([i["q_vbs2tango"] for i in im], np.float64), t=np.array([i["r_Vo2To_vbs_true"] for i in im], np.float64),
                px=np.array([i["landmarks"] for i in im], np.float64), sigma=None, valid=np.ones((5, 11), np.uint8))


def synthetic_case(N, world, seed, sigma=False, invalid=0.0, spoil=False):
    rng = np.random.default_rng(seed)
    L = len(world)
    sg = rng.uniform(0.5, 2.0, (N, L, 2)) if sigma else None
    q, t, px = lr.synthetic_views(N, world, K, seed + 1, noise=1.0, sigma=sg)
    valid = (rng.uniform(size=(N, L)) >= invalid).astype(np.uint8)
    if spoil:
        px[3, 1, 0] = np.nan
        px[4, 2, 1] = np.inf
        q[7] = 0.0
        t[9, 1] = np.nan
        sg[11, 0, 0] = np.nan
        px[70, 5] += 60.0                          # one gross outlier for the Huber branch
    return dict(q=q, t=t, px=px, sigma=sg, valid=valid)


CASES = {
    # name: (inputs, keywords)
    "n1": (lambda: synthetic_case(1, W, 1), dict()),
    "fixture_n5": (fixture_case, dict()),
    "fixture_n5_linear": (fixture_case, dict(iterations=0)),
    "n65_l1_sigma_plain": (lambda: synthetic_case(65, W[:1], 2, sigma=True), dict(huber=0.0, iterations=0)),
    "n65_l11_init": (lambda: synthetic_case(65, W, 3), dict(init=True)),
    "n130_l16_mixed": (lambda: synthetic_case(130, W16, 4, sigma=True, invalid=0.25, spoil=True), dict(sigma_gain=1.25)),
}
_cache = {}


def reference(name):
    """inputs, keywords, the forward-order restatement and the measured bound per output: computed once"""
    if name not in _cache:
        x, kw = CASES[name][0](), dict(CASES[name][1])
        init = W16[:x["px"].shape[1]] + 0.01 if kw.pop("init", False) else None
        N = len(x["q"])
        runs = [lr.solve(x["px"], x["sigma"], x["valid"], x["q"], x["t"], K, world_init=init, order=o, **kw)
                for o in (np.arange(N), np.arange(N)[::-1])]
        for k in ("status", "n_used", "obs_flags"):
            assert np.array_equal(runs[0][k], runs[1][k]), k
        spread = {k: float(np.abs(runs[0][k] - runs[1][k]).max()) for k in NUM}
        bound = {k: max(16.0 * spread[k], 1e-12 * float(np.abs(runs[0][k]).max())) for k in NUM}
        _cache[name] = (x, kw, init, runs[0], spread, bound)
    return _cache[name]


def call_solve(dev, x, init=None, iterations=10, huber=3.0, sigma_floor=1e-3, sigma_gain=1.0, z_min=0.1):
    import torch
    from spe import _lib
    N, L = x["px"].shape[:2]
    ins = [_dev(x["px"], dev), _dev(x["sigma"], dev) if x["sigma"] is not None else None, _dev(x["valid"], dev),
           _dev(x["q"], dev), _dev(x["t"], dev), _dev(K, dev), _dev(init, dev) if init is not None else None]
    nbytes = _lib.lib().spe_landmarks_scratch_bytes(N, L)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(world=torch.full((L, 3), -7.0, **f64), cov=torch.full((L, 3, 3), -7.0, **f64), chi2=torch.full((L,), -7.0, **f64),
               n_used=torch.full((L,), -7, dtype=torch.int32, device=dev), rms_px=torch.full((L,), -7.0, **f64),
               obs_flags=torch.full((N, L), 77, dtype=torch.uint8, device=dev),
               status=torch.full((L,), -7, dtype=torch.int32, device=dev))
    rc = _lib.lib().spe_landmarks_solve(
        _lib.stream_ptr(), _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), _lib.ptr(ins[3]), _lib.ptr(ins[4]), N, L,
        _lib.ptr(ins[5]), _lib.ptr(ins[6]), iterations, huber, sigma_floor, sigma_gain, z_min, _lib.ptr(scratch), nbytes,
        *[_lib.ptr(out[k]) for k in ("world", "cov", "chi2", "n_used", "rms_px", "obs_flags", "status")])
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_restatement(gpu_device, name):
    x, kw, init, ref, spread, bound = reference(name)
    rc, out = call_solve(gpu_device, x, init=init, **kw)
    assert rc == 0
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("status", "n_used", "obs_flags"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    for k in NUM:
        assert np.isfinite(got[k]).all(), k
        err = float(np.abs(got[k] - ref[k]).max())
        print(f"{name} {k}: spread {spread[k]:.3e} bound {bound[k]:.3e} kernel error {err:.3e}")
        assert err <= bound[k], (k, err, bound[k])
    if name == "n1":
        assert (got["status"] == 1).all() and not got["world"].any() and not got["obs_flags"].any()
    if name.startswith("fixture"):
        err = float(np.abs(got["world"] - W).max())
        print(name, "largest coordinate error against world_points.json", err)
        assert (got["status"] == 0).all() and err <= 1e-5
    if name == "n130_l16_mixed":
        assert (got["status"] == 0).all() and (got["obs_flags"] & 2).any()
        assert not got["obs_flags"][7].any() and not got["obs_flags"][9].any() and got["obs_flags"][3, 1] == 0


def test_degenerate_and_single_view_statuses(gpu_device):
    q, t, px = lr.synthetic_views(6, W[:4], K, seed=3)
    valid = np.ones((6, 4), np.uint8)
    valid[1:, 0] = 0
    same = dict(q=np.repeat(q[:1], 6, 0), t=np.repeat(t[:1], 6, 0), px=np.repeat(px[:1], 6, 0), sigma=None, valid=np.ones((6, 4), np.uint8))
    for x, want in ((dict(q=q, t=t, px=px, sigma=None, valid=valid), [1, 0, 0, 0]), (same, [2, 2, 2, 2])):
        ref = lr.solve(x["px"], None, x["valid"], x["q"], x["t"], K)
        rc, out = call_solve(gpu_device, x)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert rc == 0 and got["status"].tolist() == want == ref["status"].tolist()
        dead = got["status"] != 0
        for k in NUM + ("n_used",):
            assert not got[k][dead].any(), k
        assert not got["obs_flags"][:, dead].any()
        np.testing.assert_array_equal(got["obs_flags"], ref["obs_flags"])


def test_two_runs_give_the_same_bits(gpu_device):
    import torch
    x, kw, init, *_ = reference("n130_l16_mixed")
    runs = [call_solve(gpu_device, x, init=init, **kw) for _ in range(2)]
    assert runs[0][0] == 0 and runs[1][0] == 0
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k].view(torch.uint8), runs[1][1][k].view(torch.uint8)), k


def selection_inputs(B, Q, C, seed):
    """duplicate labels, exact ties and labels nobody carries"""
    rng = np.random.default_rng(seed)
    probs = rng.uniform(0.0, 0.2, (B, Q, C)).astype(np.float32)
    lab = rng.integers(0, C, (B, Q))
    score = rng.choice(np.array([0.5, 0.625, 0.75], np.float32), (B, Q))        # few values: ties are common
    probs[np.arange(B)[:, None], np.arange(Q)[None, :], lab] = score
    probs[0, :, 2] = 0.0                                                        # image 0: nobody carries label 2
    pts = rng.uniform(0, 1900, (B, Q, 2)).astype(np.float32)
    sig = rng.uniform(1e-3, 1e-2, (B, Q, 2)).astype(np.float32)
    scale = rng.uniform(200, 700, (B, 2)).astype(np.float32)
    return pts, probs, sig, scale


@pytest.mark.parametrize("Q,with_sigma", [(11, True), (30, True), (30, False)])
def test_selection_equals_the_restated_rule(gpu_device, Q, with_sigma):
    import torch
    from spe import _lib
    dev, B, C, off, rows = gpu_device, 5, 12, 3, 10
    pts, probs, sig, scale = selection_inputs(B, Q, C, 40 + Q)
    px, sg, valid = lr.select_observations(pts, probs, sig if with_sigma else None, scale if with_sigma else None)
    assert valid.min() == 0 and valid.max() == 1
    out = [torch.full((rows, C - 1, 2), -7.0, dtype=torch.float64, device=dev),
           torch.full((rows, C - 1, 2), -7.0, dtype=torch.float64, device=dev),
           torch.full((rows, C - 1), 77, dtype=torch.uint8, device=dev)]
    d = [_dev(a, dev) for a in (pts, probs, sig, scale)]
    rc = _lib.lib().spe_landmark_observations(
        _lib.stream_ptr(), _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2] if with_sigma else None),
        _lib.ptr(d[3] if with_sigma else None), B, Q, C, off, *[_lib.ptr(o) for o in out])
    torch.cuda.synchronize()
    assert rc == 0
    got = [o.cpu().numpy() for o in out]
    for g, r, name in zip(got, (px, sg, valid), ("obs_px", "obs_sigma", "obs_valid")):
        np.testing.assert_array_equal(g[off:off + B], r, err_msg=name)
        untouched = np.concatenate([g[:off], g[off + B:]])
        assert (untouched == (77 if name == "obs_valid" else -7.0)).all(), name


def test_evaluate_rtdetr_feeds_the_reconstruction(gpu_device, tmp_path):
    """64 images in two batches of a stand-in model, 1 sigma of noise on crop-normalised sigmas, through
    evaluate_rtdetr(landmarks=rec): the solved table is within 3 sqrt(diag cov_scaled) of the truth for at least
    10 of 11 landmarks, equals the restatement on the same observations, leaves the evaluation's log as it is
    without it, and round-trips through save() into a solver's world=."""
    import torch
    from spe.engine import evaluate_rtdetr
    from spe.landmarks import LandmarkReconstruction
    from spe.solver import SimplePoseSolverSigma, build_solver
    dev, N, B, Q = gpu_device, 64, 32, 30
    d = lr.model_outputs(N, W, K, seed=21, Q=Q)
    names = [f"img{i}.jpg" for i in range(N)]
    gt = {n: {"quat": d["q"][i].tolist(), "tvec": d["t"][i].tolist()} for i, n in enumerate(names)}
    loader = [(torch.zeros(B, 3, 8, 8), [{"filename": names[i], "clip_bbox": torch.from_numpy(d["clip"][i])}
                                         for i in range(k * B, k * B + B)]) for k in range(N // B)]

    def model(samples, clip_bbox=None):
        k = [i for i in range(N // B) if np.array_equal(clip_bbox.cpu().numpy(), d["clip"][i * B:i * B + B])][0]
        s = slice(k * B, k * B + B)
        z = torch.zeros(B, Q, 12, device=dev)
        return {"points_px": _dev(d["points"][s], dev), "probs": _dev(d["probs"][s], dev), "sigmas": _dev(d["sigmas"][s], dev),
                "pred_logits": z, "aux_outputs": [{"pred_logits": z} for _ in range(3)]}

    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma"))
    rec = LandmarkReconstruction(11)
    sp, ep = evaluate_rtdetr(model, None, None, loader, gt, solver, dev)
    sl, el = evaluate_rtdetr(model, None, None, loader, gt, solver, dev, landmarks=rec)
    assert el.log == ep.log and sl == sp and rec.n == N
    m = rec.solve()
    px, sg, valid = lr.select_observations(d["points"], d["probs"], d["sigmas"], d["scale"])
    obs = {k: v.cpu().numpy() for k, v in rec.observations().items()}
    np.testing.assert_array_equal(obs["obs_px"], px)
    np.testing.assert_array_equal(obs["obs_sigma"], sg)
    np.testing.assert_array_equal(obs["obs_valid"], valid)
    ref = lr.solve(px, sg, valid, d["q"], d["t"], K)
    rev = lr.solve(px, sg, valid, d["q"], d["t"], K, order=np.arange(N)[::-1])
    bound = max(16.0 * float(np.abs(ref["world"] - rev["world"]).max()), 1e-12 * float(np.abs(ref["world"]).max()))
    ok = lr.within_3_sigma(m.points, m.cov, m.chi2, m.n_used, W)
    np.testing.assert_array_equal(ok, (np.abs(m.points - W) <= 3 * np.sqrt(np.diagonal(m.cov_scaled, axis1=1, axis2=2))).all(1))
    print("within 3 sigma:", int(ok.sum()), "of 11; largest distance", m.compare(W).max(), "against the restatement",
          np.abs(m.points - ref["world"]).max(), "birge", m.birge().max())
    assert (m.status == 0).all() and ok.sum() >= 10
    np.testing.assert_array_equal(m.obs_flags, ref["obs_flags"])
    assert np.abs(m.points - ref["world"]).max() <= bound
    # the table into a solver: the packaged one as world= changes no bit, the solved one moves the poses a little
    path = tmp_path / "solved.json"
    m.save(str(path))
    ins = [_dev(d[k][:B], dev) for k in ("points", "probs", "sigmas")]
    base = SimplePoseSolverSigma().solve_batch(*ins)
    same = SimplePoseSolverSigma(world=world_points()).solve_batch(*ins)
    for k in ("quat", "tvec", "rvec", "status", "inlier_mask"):
        assert torch.equal(base[k], same[k]), k
    mine = build_solver(argparse.Namespace(solver="epnp_ransac_sigma", world=str(path)))
    assert np.array_equal(mine.W_Pt, m.points)
    moved = mine.solve_batch(*ins)
    assert (moved["tvec"] - base["tvec"]).abs().max().item() > 0
    s2 = SimplePoseSolverSigma()
    s2.solve_batch(*ins)
    s2.set_world(m)
    assert torch.equal(s2.solve_batch(*ins)["tvec"], moved["tvec"])


def test_annotations_on_the_real_images_and_growth(gpu_device):
    """update_annotations on the five real images, one image per call into buffers that must grow (a first
    capacity of 2 is forced), gives the kernel test's answer; init= takes a LandmarkModel."""
    from spe.landmarks import LandmarkReconstruction
    x = fixture_case()
    rec = LandmarkReconstruction(11)
    rec.update_annotations(x["px"][:1], x["q"][:1], x["t"][:1])
    rec._buf = {k: v[:2].clone() for k, v in rec._buf.items()}
    for i in range(1, 5):
        rec.update_annotations(_dev(x["px"][i:i + 1], gpu_device), x["q"][i:i + 1], x["t"][i:i + 1],
                               valid=np.ones((1, 11), np.uint8))
    assert rec.n == 5 and rec._buf["q"].shape[0] >= 5
    m = rec.solve()
    ref = reference("fixture_n5")[3]
    assert (m.status == 0).all() and np.abs(m.points - W).max() <= 1e-5
    assert np.abs(m.points - ref["world"]).max() <= reference("fixture_n5")[5]["world"]
    m0 = rec.solve(iterations=0, init=m)
    assert np.array_equal(m0.points, m.points) and (m0.status == 0).all()
