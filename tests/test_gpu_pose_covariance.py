"""GPU: spe_pose_covariance (csrc/pnp.hip pose_cov_kernel) against tests/pose_covariance_ref.py on poses
that spe_pnp_batch itself (sigma mode) solved from synthetic keypoints, plus the status rules, determinism,
the argument refusals and PosePipeline(pose_cov=True).

Tolerance of the covariance, both sides fp64 (the kernel and the reference differ in the rotation
matrix by a rounding, in the order of the sum and in how they invert):
    |cov_gpu - cov_ref| <= 64 eps kappa max|cov_ref|,   kappa = cond(D^-1/2 H D^-1/2) from the reference alone.
The inputs are chosen (seeds below, checked on the CPU at the true poses when this was written) so that
kappa <= 1e8 on every image with status 0; the test asserts that too and prints the largest.  The
information matrix rebuilt from the kernel's covariance, inv(D^1/2 cov D^1/2) in numpy, is compared with
the reference's scaled H to 6 * 64 eps kappa^2 (entries of a 6x6 of unit diagonal): the covariance's
relative error 64 eps kappa grows by one more factor kappa through the inversion, 6 bounds the row sums.
The derived outputs are checked against the kernel's own covariance to a rounding of their format.
cov_status is compared exactly and no image is skipped.
"""
import argparse
import functools

import numpy as np
import pytest

import pose_covariance_ref as pc
import postmodel_ref as pr

pytestmark = pytest.mark.gpu

SPE_E_ARG = -1
FILL = -7
EPS = np.finfo(np.float64).eps
OUT = ("cov", "sigma_rot", "sigma_t", "pred_score", "cov_status")

# (B, Q, C): B = 5 is no multiple of the 4 images of a work-group, 257 leaves a one-image tail block;
# Q = 64 fills the wave, C = 17 gives 16 correspondences (every lane of the sum's tree)
SHAPES = [(1, 11, 12), (5, 30, 17), (257, 64, 17), (257, 30, 12), (5, 11, 17)]
COUNTS = (3, 4, 11, 16)


def _dev(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def call_cov(dev, probs, sig, status, corr_label, mask, rvec, tvec, C_world, scale=None, floor=1e-3, Q=None, C=None):
    """spe_pose_covariance through ctypes on numpy inputs; outputs start filled with a sentinel.
    -> rc, dict of device tensors."""
    import torch
    from spe import _lib
    from spe.config import Camera
    B, q, c = probs.shape
    out = dict(cov=torch.full((B, 6, 6), FILL, dtype=torch.float64, device=dev),
               sigma_rot=torch.full((B,), FILL, dtype=torch.float32, device=dev),
               sigma_t=torch.full((B, 3), FILL, dtype=torch.float64, device=dev),
               pred_score=torch.full((B,), FILL, dtype=torch.float32, device=dev),
               cov_status=torch.full((B,), FILL, dtype=torch.int32, device=dev))
    ins = [_dev(probs, dev), _dev(sig, dev), _dev(scale, dev), _dev(np.asarray(status, np.int32), dev),
           _dev(np.asarray(corr_label, np.int32), dev), _dev(np.asarray(mask, np.uint32).view(np.int32), dev),
           _dev(np.asarray(rvec, np.float64), dev), _dev(np.asarray(tvec, np.float64), dev)]
    K, W = _dev(Camera.K, dev), _dev(pr.world_for(C_world), dev)
    rc = _lib.lib().spe_pose_covariance(_lib.stream_ptr(), *[_lib.ptr(a) for a in ins], B, q if Q is None else Q,
                                        c if C is None else C, _lib.ptr(K), _lib.ptr(W), floor,
                                        *[_lib.ptr(out[k]) for k in OUT])
    torch.cuda.synchronize()
    return rc, out


def _untouched(out):
    return all(bool((t == FILL).all()) for t in out.values())


def inputs(B, Q, C):
    """The case's keypoints and sigma scales (numpy; deterministic)."""
    from spe.config import Camera
    pts, probs, sig, R, t = pc.keypoint_set(B, Q, C, pr.world_for(C), Camera.K, seed=1000 * B + 10 * Q + C)
    scale = np.random.default_rng(B + Q + C).uniform(0.5, 4.0, (B, 2)).astype(np.float32)
    return pts, probs, sig, scale


@functools.lru_cache(maxsize=None)
def solved(B, Q, C):
    """spe_pnp_batch (EPnP-RANSAC + sigma LM) on the case's keypoints, once per case, with the inlier
    masks doctored to 3 / 4 / 11 / 16 inliers in turn where the image has that many correspondences."""
    import torch
    from spe import _lib
    from spe.config import Camera
    dev = torch.device("cuda:0")
    pts, probs, sig, scale = inputs(B, Q, C)
    out = dict(quat=torch.empty(B, 4, device=dev), tvec=torch.empty(B, 3, dtype=torch.float64, device=dev),
               rvec=torch.empty(B, 3, dtype=torch.float64, device=dev), status=torch.empty(B, dtype=torch.int32, device=dev),
               n_corr=torch.empty(B, dtype=torch.int32, device=dev),
               corr_label=torch.empty(B, 16, dtype=torch.int32, device=dev),
               inlier_mask=torch.empty(B, dtype=torch.int32, device=dev))
    ins = [_dev(pts, dev), _dev(probs, dev), _dev(sig, dev)]
    K, W = _dev(Camera.K, dev), _dev(pr.world_for(C), dev)
    rc = _lib.lib().spe_pnp_batch(_lib.stream_ptr(), *[_lib.ptr(a) for a in ins], B, Q, C, _lib.ptr(K), _lib.ptr(W), 2,
                                  25.0, 100, 0.99, *[_lib.ptr(out[k]) for k in ("quat", "tvec", "rvec", "status", "n_corr",
                                                                                  "corr_label", "inlier_mask")], None)
    assert rc == 0
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in out.items()}
    h["solver_mask"] = h["inlier_mask"].view(np.uint32).copy()
    h["inlier_mask"] = pc.doctor_masks(h["solver_mask"], h["n_corr"], COUNTS, seed=B + Q)
    return h


def check_against_reference(got, ref, tvec, what):
    """Device outputs (numpy) against the reference dict: -> the largest kappa among the status-0 images."""
    np.testing.assert_array_equal(got["cov_status"], ref["cov_status"], err_msg=str(what))
    ok = ref["cov_status"] == 0
    assert np.isfinite(got["cov"]).all() and np.isfinite(got["sigma_t"]).all()
    for k in ("cov", "sigma_rot", "sigma_t", "pred_score"):
        assert not got[k][~ok].any(), (what, k)
    worst = 0.0
    for b in np.nonzero(ok)[0]:
        kappa = ref["kappa"][b]
        assert kappa <= 1e8, (what, b, kappa)
        c, r = got["cov"][b], ref["cov"][b]
        np.testing.assert_array_equal(c, c.T)
        bound = 64 * EPS * kappa * np.abs(r).max()
        err = np.abs(c - r).max()
        worst = max(worst, err / bound)
        assert err <= bound, (what, b, err, bound, kappa)
        d = np.sqrt(np.diag(ref["H"][b]))
        S_ref = ref["H"][b] / np.outer(d, d)
        S_gpu = np.linalg.inv(c * np.outer(d, d))
        assert np.abs(S_gpu - S_ref).max() <= 6 * 64 * EPS * kappa ** 2, (what, b, kappa)
        tr_w, tr_t = np.trace(c[:3, :3]), np.trace(c[3:, 3:])
        np.testing.assert_allclose(got["sigma_rot"][b], np.sqrt(tr_w), rtol=2.0 ** -23)
        np.testing.assert_allclose(got["sigma_t"][b], np.sqrt(np.diag(c)[3:]), rtol=4 * EPS)
        np.testing.assert_allclose(got["pred_score"][b], np.sqrt(tr_w) + np.sqrt(tr_t) / np.linalg.norm(tvec[b]),
                                   rtol=2.0 ** -23)
    kmax = float(np.nanmax(ref["kappa"][ok])) if ok.any() else 0.0
    print(what, "status-0 images:", int(ok.sum()), "largest kappa: %.3g" % kmax, "largest error / bound: %.3g" % worst)
    return kmax


def to_numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("scaled", [False, True], ids=["px", "scaled"])
@pytest.mark.parametrize("B,Q,C", SHAPES)
def test_kernel_matches_reference_on_solver_poses(gpu_device, B, Q, C, scaled):
    from spe.config import Camera
    pts, probs, sig, scale = inputs(B, Q, C)
    h = solved(B, Q, C)
    sc = scale if scaled else None
    rc, out = call_cov(gpu_device, probs, sig, h["status"], h["corr_label"], h["inlier_mask"], h["rvec"], h["tvec"], C, sc)
    assert rc == 0
    ref = pc.pose_covariance(probs, sig, h["status"], h["corr_label"], h["inlier_mask"], h["rvec"], h["tvec"], Camera.K,
                             pr.world_for(C), sigma_scale=sc)
    check_against_reference(to_numpy(out), ref, h["tvec"], (B, Q, C, scaled))
    ok = ref["cov_status"] == 0
    # 0.3 px of noise, no outliers, at least 3 inliers kept: the solver solves every image and every image
    # has a covariance, so the case cannot thin out
    assert (h["status"] == 0).all() and ok.all()
    if B == 257:
        n = np.array([bin(int(m)).count("1") for m in h["inlier_mask"]])
        for want in COUNTS:
            if want <= min(Q, C - 1):
                assert ((n == want) & ok).any(), want               # every forced inlier count among the status-0 images
        assert ok[256]                                             # the tail block's image
    # the tied duplicate of keypoint_set is in every image with Q > C - 1: the selection's tie rule decides
    # which sigma enters, so a wrong rule shows as a covariance error above


def _stack(cases):
    keys = ("probs", "sigmas", "status", "corr_label", "inlier_mask", "rvec", "tvec")
    return {k: np.concatenate([c[k] for c in cases]) for k in keys}


def mixed_batch():
    """The CPU test's status cases (pose_covariance_ref.status_cases), every non-zero status among them,
    between good images: -> stacked inputs, expected statuses."""
    cases = pc.status_cases()
    good = [pc.one_image(*pc.pose(40 + i, z=6.0 + i), np.full((11, 2), 0.2 + 0.1 * i, np.float32)) for i in range(5)]
    order, want = [], []
    for i, (name, (inp, st)) in enumerate(cases.items()):
        order.append(good[i % len(good)])
        want.append(0)
        order.append(inp)
        want.append(st)
    return _stack(order), np.array(want, np.int32)


def test_status_rules_in_a_mixed_batch(gpu_device):
    from spe.config import Camera
    x, want = mixed_batch()
    assert set(want) == {0, 1, 2, 3, 4}
    args = lambda d: (d["probs"], d["sigmas"], d["status"], d["corr_label"], d["inlier_mask"], d["rvec"], d["tvec"])
    rc, out = call_cov(gpu_device, *args(x), 12)
    assert rc == 0
    got = to_numpy(out)
    np.testing.assert_array_equal(got["cov_status"], want)
    ref = pc.pose_covariance(*args(x), Camera.K, pr.world_for(12))
    check_against_reference(got, ref, x["tvec"], "mixed")
    # the good images alone: the same bits as beside the bad ones
    keep = np.nonzero(want == 0)[0]
    rc, alone = call_cov(gpu_device, *[a[keep] for a in args(x)], 12)
    assert rc == 0
    for k in OUT:
        np.testing.assert_array_equal(alone[k].cpu().numpy(), got[k][keep], err_msg=k)


def test_two_runs_give_the_same_bits(gpu_device):
    import torch
    B, Q, C = 257, 64, 17
    pts, probs, sig, scale = inputs(B, Q, C)
    h = solved(B, Q, C)
    runs = [call_cov(gpu_device, probs, sig, h["status"], h["corr_label"], h["inlier_mask"], h["rvec"], h["tvec"], C, scale)
            for _ in range(2)]
    assert runs[0][0] == 0 and runs[1][0] == 0
    for k in OUT:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


@pytest.mark.parametrize("case", ["q65", "c18", "floor0"])
def test_refusals_leave_the_outputs_alone(gpu_device, case):
    from spe import _lib
    B, Q, C = 5, 30, 17
    pts, probs, sig, scale = inputs(B, Q, C)
    h = solved(B, Q, C)
    kw = {"q65": dict(Q=65), "c18": dict(C=18), "floor0": dict(floor=0.0)}[case]
    rc, out = call_cov(gpu_device, probs, sig, h["status"], h["corr_label"], h["inlier_mask"], h["rvec"], h["tvec"], C,
                       **kw)
    assert rc == SPE_E_ARG and _lib.lib().spe_last_error()
    assert _untouched(out)


# ---------------------------------------------------------------- the Python layer on solved poses
# A model with random weights gives the solver nothing to solve, and a covariance path that only ever
# takes the no-pose exit compares zeros with zeros.  The cases below put synthetic keypoints
# (pose_covariance_ref.keypoint_set) where the model's post-processed outputs go, with the sigmas
# crop-normalised as a model emits them: sigma_px / (crop width, crop height) of the box the forward was
# given.  The reference then gets sigma_scale = that box's width and height, so a swapped axis, an unscaled
# sigma or another batch's box moves the covariance by far more than the bound.


def _boxes(B, seed):
    """B crop boxes (x1, y1, x2, y2), float32, width != height."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 600, (B, 2))
    wh = np.stack([rng.uniform(200, 400, B), rng.uniform(450, 700, B)], 1)
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def _scale_of(clip):
    clip = np.asarray(clip, np.float32)
    return np.stack([clip[:, 2] - clip[:, 0], clip[:, 3] - clip[:, 1]], 1)


def _synthetic_outputs(B, Q, seed, clip):
    """(points_px, probs, crop-normalised sigmas) float32 for the boxes `clip`, C = 12."""
    from spe.config import Camera
    pts, probs, sig, R, t = pc.keypoint_set(B, Q, 12, pr.world_for(12), Camera.K, seed=seed)
    return pts, probs, (sig / _scale_of(clip)[:, None, :]).astype(np.float32)


def _check_python_layer(cov, probs, sig_n, poses, clip, what):
    """A pose_covariance dict (device) against the reference with sigma_scale = the boxes' width and
    height; every image must have a covariance."""
    from spe.config import Camera
    h = {k: poses[k].cpu().numpy() for k in ("status", "corr_label", "inlier_mask", "rvec", "tvec")}
    ref = pc.pose_covariance(probs, sig_n, h["status"], h["corr_label"], h["inlier_mask"].view(np.uint32), h["rvec"],
                             h["tvec"], Camera.K, pr.world_for(12), sigma_scale=_scale_of(clip))
    got = {"cov": cov["pose_cov"].cpu().numpy(), **{k: cov[k].cpu().numpy() for k in OUT[1:]}}
    assert (got["cov_status"] == 0).all(), (what, got["cov_status"])
    check_against_reference(got, ref, h["tvec"], what)
    return ref


class _Doctored:
    """An RTDETR whose post-processed outputs are overwritten, on the stream they were made on, with the
    synthetic keypoints of the batch whose crop boxes the forward was given."""

    def __init__(self, model, batches, dev):
        self.m = model
        self.batches = [(torch_clip, [_dev(a, dev) for a in arrays]) for torch_clip, arrays in batches]

    def __getattr__(self, k):
        return getattr(self.m, k)

    def _doctor(self, fo, clip_bbox):
        import torch
        hit = [arrays for c, arrays in self.batches if torch.equal(c, clip_bbox)]
        assert len(hit) == 1, "the forward got none of the loaded crop boxes"
        for k, a in zip(("points_px", "probs", "sigmas"), hit[0]):
            fo[k].copy_(a)
        return fo

    def __call__(self, images, clip_bbox=None, **kw):
        return self._doctor(self.m(images, clip_bbox=clip_bbox, **kw), clip_bbox)

    def decode(self, B, ws, clip_bbox=None, **kw):
        return self._doctor(self.m.decode(B, ws, clip_bbox=clip_bbox, **kw), clip_bbox)


def test_pipeline_carries_the_covariance(gpu_device):
    """PosePipeline(pose_cov=True) on a small RT-DETR (r18, S = 128, B = 3), plain and overlap_backbone, two
    batches with different crop boxes run back to back (in the staged mode both are in flight, each in its
    slot): every image is solved and has a covariance, which is the reference's for that batch's boxes and
    solver.pose_covariance's by hand; with pose_cov off every other output is the same."""
    import torch
    from spe.pipeline import PosePipeline
    from spe.rtdetr import RTDETR
    from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights
    from spe.solver import build_solver
    dev, B, S = gpu_device, 3, 128
    cfg = RtdetrConfig(depth=18, input_size=S)
    real = RTDETR(cfg, dtype="bf16")
    real.load_state_dict(random_rtdetr_weights(cfg, 0))
    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma"))
    g = torch.Generator().manual_seed(5)
    images = torch.randn(B, 3, S, S, generator=g).to(dev)
    clips = [_boxes(B, 70 + k) for k in range(2)]
    synth = [_synthetic_outputs(B, cfg.num_queries, 80 + k, clips[k]) for k in range(2)]
    dclips = [_dev(c, dev) for c in clips]
    m = _Doctored(real, list(zip(dclips, synth)), dev)
    new = ("pose_cov", "pred_score", "sigma_t", "sigma_rot", "cov_status")

    def flat(o, prefix=""):
        for k, v in (o.items() if isinstance(o, dict) else enumerate(o)):
            if torch.is_tensor(v):
                yield f"{prefix}{k}", v
            elif isinstance(v, (dict, list, tuple)):
                yield from flat(v, f"{prefix}{k}.")

    for kw in ({}, dict(overlap_backbone=True)):
        outs = {}
        for on in (False, True):
            p = PosePipeline(m, solver, B, device=dev, pose_cov=on, **kw)
            res = []
            for k in range(2):
                p.load(images, dclips[k])
                res.append(p.run())
            for o in res:
                p.wait(o)
            torch.cuda.synchronize()
            outs[on] = res
        for k in range(2):
            off, on = outs[False][k], outs[True][k]
            assert not any(n in off for n in new) and all(n in on for n in new)
            a = dict(flat({n: v for n, v in off.items() if n != "stream"}))
            b = dict(flat({n: v for n, v in on.items() if n != "stream" and n not in new}))
            assert a.keys() == b.keys()
            for n in a:
                assert torch.equal(a[n], b[n]), (kw, k, n)
            assert (on["poses"]["status"] == 0).all()
            _check_python_layer(on, synth[k][1], synth[k][2], on["poses"], clips[k], ("pipeline", kw, k))
            hand = solver.pose_covariance(on["forward"]["probs"], on["forward"]["sigmas"], on["poses"], clip_bbox=dclips[k])
            torch.cuda.synchronize()
            for n in new:
                assert torch.equal(on[n], hand[n]), (kw, k, n)
        assert not torch.equal(outs[True][0]["pose_cov"], outs[True][1]["pose_cov"])


@pytest.mark.parametrize("solver_name", ["epnp_ransac_sigma", "exhaustive", "epnp_ceres"])
def test_solver_method_scales_by_the_crop(gpu_device, solver_name):
    """PoseSolver.pose_covariance(clip_bbox=...) on the solve_batch output of the RANSAC sigma, the
    exhaustive and the Ceres-style solver classes, against the reference with sigma_scale = (width, height)."""
    import torch
    from spe.solver import build_solver
    B, Q = 5, 30
    clip = _boxes(B, 91)
    pts, probs, sig_n = _synthetic_outputs(B, Q, 92, clip)
    solver = build_solver(argparse.Namespace(solver=solver_name))
    d = [_dev(a, gpu_device) for a in (pts, probs, sig_n)]
    kw = dict(area=[200.0] * B) if solver_name == "epnp_ceres" else {}
    poses = solver.solve_batch(*d, **kw)
    cov = solver.pose_covariance(d[1], d[2], poses, clip_bbox=_dev(clip, gpu_device))
    torch.cuda.synchronize()
    assert (poses["status"] == 0).all()
    _check_python_layer(cov, probs, sig_n, poses, clip, solver_name)


def test_evaluate_rtdetr_records_the_predicted_score(gpu_device):
    """evaluate_rtdetr(pose_cov=True) over two batches of a stand-in model that returns synthetic outputs
    on the device: every record carries cov_status 0 and the reference's pred_score for its own crop box
    (float32, rounded to 8 decimals); without pose_cov no record has either field."""
    import torch
    from spe.engine import evaluate_rtdetr
    from spe.solver import build_solver
    dev, B, Q = gpu_device, 3, 30
    names = [f"img{i}.jpg" for i in range(2 * B)]
    gt = {n: {"quat": [1.0, 0.0, 0.0, 0.0], "tvec": [0.0, 0.0, 8.0]} for n in names}
    clips = [_boxes(B, 60 + k) for k in range(2)]
    synth = [_synthetic_outputs(B, Q, 50 + k, clips[k]) for k in range(2)]
    loader = [(torch.zeros(B, 3, 8, 8), [{"filename": names[k * B + b], "clip_bbox": torch.from_numpy(clips[k][b])}
                                         for b in range(B)]) for k in range(2)]
    seen = []

    def model(samples, clip_bbox=None):
        k = [i for i in range(2) if np.array_equal(clip_bbox.cpu().numpy(), clips[i])][0]
        pts, probs, sig = [_dev(a, dev) for a in synth[k]]
        seen.append((k, pts, probs, sig))
        z = torch.zeros(B, Q, 12, device=dev)
        return {"points_px": pts, "probs": probs, "sigmas": sig, "pred_logits": z,
                "aux_outputs": [{"pred_logits": z} for _ in range(3)]}

    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma"))
    stats, ev = evaluate_rtdetr(model, None, None, loader, gt, solver, dev, pose_cov=True)
    assert list(ev.log) == names
    for k, pts, probs, sig in seen:
        poses = solver.solve_batch(pts, probs, sig)
        torch.cuda.synchronize()
        cov = solver.pose_covariance(probs, sig, poses, clip_bbox=_dev(clips[k], dev))
        ref = _check_python_layer(cov, synth[k][1], synth[k][2], poses, clips[k], ("evaluate", k))
        for b in range(B):
            rec = ev.log[names[k * B + b]]
            assert rec["cov_status"] == 0
            assert abs(rec["pred_score"] - ref["pred_score"][b]) <= 2.0 ** -22 * ref["pred_score"][b] + 1e-8
    stats, ev = evaluate_rtdetr(model, None, None, loader, gt, solver, dev)
    assert not any("pred_score" in r or "cov_status" in r for r in ev.log.values())


def test_generate_submission_records_the_predicted_score(gpu_device):
    """generate_submission(pose_cov=True) from 3 JPEG files (batch size 2, a short last batch, one box
    partly outside the frame) through the real decoder and crop transform, with a stand-in model that
    returns synthetic outputs for the crop boxes it is handed: each record's pred_score is the reference's
    for the transform's own clip_bbox, cov_status 0; without pose_cov the records are as before."""
    import io
    import torch
    from PIL import Image
    from spe.datasets import JpegDecoder
    from spe.engine import generate_submission
    from spe.solver import build_solver
    dev, Q = gpu_device, 30
    rng = np.random.default_rng(23)
    H, W = 1200, 1920
    names = ["img3.jpg", "img1.jpg", "img2.jpg"]
    files = {}
    for n in names:
        bio = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (H, W), dtype=np.uint8)).save(bio, "JPEG", quality=50)
        files[n] = bio.getvalue()
    boxes = [[700.0, 300.0, 1300.0, 900.0], [-60.5, 200.0, 500.0, 850.0], [900.2, 410.9, 1400.4, 700.1]]
    anns = {n: [b + [0.9]] for n, b in zip(names, boxes)}
    dec = JpegDecoder(H, W, max_bytes=max(map(len, files.values())))
    calls = []

    def model(crops, clip_bbox=None):
        clip = clip_bbox.cpu().numpy()
        pts, probs, sig_n = _synthetic_outputs(len(clip), Q, 30 + len(calls), clip)
        calls.append((clip, pts, probs, sig_n))
        return {"points_px": _dev(pts, dev), "probs": _dev(probs, dev), "sigmas": _dev(sig_n, dev)}

    solver = build_solver(argparse.Namespace(solver="epnp_ransac_sigma"))
    log = generate_submission(model, None, anns, files.__getitem__, solver, dev, 2, 256, decoder=dec, pose_cov=True)
    assert list(log) == names and [len(c[0]) for c in calls] == [2, 1]
    i = 0
    for clip, pts, probs, sig_n in calls:
        d = [_dev(a, dev) for a in (pts, probs, sig_n)]
        poses = solver.solve_batch(*d)
        cov = solver.pose_covariance(d[1], d[2], poses, clip_bbox=_dev(clip, dev))
        torch.cuda.synchronize()
        ref = _check_python_layer(cov, probs, sig_n, poses, clip, ("submission", i))
        for b in range(len(clip)):
            rec = log[names[i]]
            assert set(rec) == {"quat_pr", "tvec_pr", "pred_score", "cov_status"} and rec["cov_status"] == 0
            assert abs(rec["pred_score"] - ref["pred_score"][b]) <= 2.0 ** -22 * ref["pred_score"][b] + 1e-8
            i += 1
    n_before = len(calls)
    plain = generate_submission(model, None, anns, files.__getitem__, solver, dev, 2, 256, decoder=dec)
    assert len(calls) == n_before + 2
    assert all(set(r) == {"quat_pr", "tvec_pr"} for r in plain.values())
