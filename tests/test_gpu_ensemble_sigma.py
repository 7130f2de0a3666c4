"""GPU: spe_ensemble_fuse_sigma (csrc/ensemble.hip ensemble_fuse_sigma_kernel) against
tests/ensemble_sigma_ref.py, its determinism and refusals, SigmaEnsemblePoseSolver over every backend and
generate_submission with a list of sigma models.

Tolerance.  The counts and the row order are compared exactly.  Every float32 output must lie within one
float32 ulp of the restatement's fp64 value rounded to float32: both sides do the same few dozen fp64
operations in the same order, whose error is far below a float32 ulp, so only the final rounding can
differ.  A gate decision taken within rounding of `gate` could go either way on the two sides; the inputs'
seeds are chosen so that every decision of the restatement is at least 1e-6 from it, which each case asserts.
"""
import argparse
import functools

import numpy as np
import pytest

import ensemble_sigma_ref as es
import postmodel_ref as pr

pytestmark = pytest.mark.gpu

SPE_E_ARG = -1
FILL = -7
OUT = ("points", "probs", "sigmas", "n_pooled", "n_kept")
FLOOR, GATE = 0.05, 3.0

# (M, B, Q, C, scaled): the smallest problem; two models, labels and queries no power of two; B = 65 puts an
# image past a multiple of 64; M = 16 with M * Q = 256 and K = 16, both limits; sigma_scale
CASES = [(1, 1, 1, 2, False), (2, 3, 11, 12, False), (3, 65, 30, 12, False), (16, 2, 16, 17, False),
         (5, 4, 30, 12, True)]


def _dev(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def case(M, B, Q, C, scaled):
    """The case's inputs and the restatement's result, computed once."""
    pts, probs, sig, scale = es.ensemble_inputs(M, B, Q, C, seed=100 * M + 10 * B + Q + C, scaled=scaled)
    ref = es.fuse_batch(pts, probs, sig, scale, sigma_floor=FLOOR, gate=GATE)
    return pts, probs, sig, scale, ref


def call_fuse(dev, pts, probs, sig, scale=None, floor=FLOOR, gate=GATE, M=None, Q=None, C=None, no_sigmas=False):
    """spe_ensemble_fuse_sigma through ctypes on numpy inputs; the outputs start filled with a sentinel and
    have the arrays' own shape whatever sizes the call names.  -> rc, dict of device tensors."""
    import torch
    from spe import _lib
    m, B, q, c = probs.shape
    K = c - 1
    out = dict(points=torch.full((B, K, 2), FILL, dtype=torch.float32, device=dev),
               probs=torch.full((B, K, c), FILL, dtype=torch.float32, device=dev),
               sigmas=torch.full((B, K, 2), FILL, dtype=torch.float32, device=dev),
               n_pooled=torch.full((B, K), FILL, dtype=torch.int32, device=dev),
               n_kept=torch.full((B, K), FILL, dtype=torch.int32, device=dev))
    ins = [_dev(pts, dev), _dev(probs, dev), None if no_sigmas else _dev(sig, dev), _dev(scale, dev)]
    rc = _lib.lib().spe_ensemble_fuse_sigma(_lib.stream_ptr(), *[_lib.ptr(a) for a in ins], m if M is None else M, B,
                                            q if Q is None else Q, c if C is None else C, floor, gate,
                                            *[_lib.ptr(out[k]) for k in OUT])
    torch.cuda.synchronize()
    return rc, out


def within_one_ulp(got, want64):
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize("M,B,Q,C,scaled", CASES)
def test_kernel_matches_the_restatement(gpu_device, M, B, Q, C, scaled):
    pts, probs, sig, scale, ref = case(M, B, Q, C, scaled)
    assert ref["min_margin"] >= 1e-6, ref["min_margin"]
    rc, out = call_fuse(gpu_device, pts, probs, sig, scale)
    assert rc == 0
    got = {k: v.cpu().numpy() for k, v in out.items()}
    np.testing.assert_array_equal(got["n_pooled"], ref["n_pooled"])
    np.testing.assert_array_equal(got["n_kept"], ref["n_kept"])
    K = C - 1
    for b in range(B):                                     # row order: the label is the row's only non-zero column
        n = len(ref["labels"][b])
        assert [int(np.flatnonzero(got["probs"][b, i])[0]) for i in range(n)] == ref["labels"][b], b
        assert (np.count_nonzero(got["probs"][b], axis=1) == 1).all()
        assert (got["probs"][b, n:, K] == 1).all()
    worst = 0.0
    for k in ("points", "probs", "sigmas"):
        assert np.isfinite(got[k]).all(), k
        ok = within_one_ulp(got[k], ref[k])
        worst = max(worst, float(np.abs(got[k] - ref[k]).max()))
        assert ok.all(), (k, np.argwhere(~ok)[:5])
    print((M, B, Q, C, scaled), "smallest gate margin %.3g" % ref["min_margin"], "largest |gpu - fp64| %.3g" % worst,
          "gated rows", int((ref["n_kept"] < ref["n_pooled"]).sum()))
    if M >= 3:
        # the case holds what it is there for: a gated outlier, a left-out measurement, a floored sigma,
        # a label that not every model carries, an image without any
        assert (ref["n_kept"] < ref["n_pooled"]).any()
        assert ((ref["n_pooled"] > 0) & (ref["n_pooled"] < M)).any()
        assert not ref["labels"][B - 1] and not got["points"][B - 1].any() and not got["sigmas"][B - 1].any()
    if M == 16:
        assert (ref["n_pooled"] - ref["n_kept"] >= 2).any()   # two gate passes on one label


def test_the_inputs_hold_every_special_case():
    """On the CPU side of the largest 12-class case: an infinite and a NaN sigma, a sigma below the floor
    and a tied score are among the selected measurements."""
    pts, probs, sig, scale, ref = case(3, 65, 30, 12, False)
    seen = set()
    for b in range(65):
        for l, recs in es.measurements(pts[:, b], probs[:, b], sig[:, b], None, FLOOR).items():
            for r in recs:
                s = sig[r["m"], b, r["q"]]
                seen |= {"inf"} if np.isinf(s).any() else set()
                seen |= {"nan"} if np.isnan(s).any() else set()
                seen |= {"floor"} if (s < FLOOR).any() else set()
                ties = [q for q in range(30) if q != r["q"] and np.array_equal(probs[r["m"], b, q], probs[r["m"], b, r["q"]])]
                seen |= {"tie"} if ties and min(ties) > r["q"] else set()
    assert seen == {"inf", "nan", "floor", "tie"}


def test_two_runs_give_the_same_bits(gpu_device):
    import torch
    pts, probs, sig, scale, ref = case(5, 4, 30, 12, True)
    a, b = (call_fuse(gpu_device, pts, probs, sig, scale) for _ in range(2))
    assert a[0] == 0 and b[0] == 0
    for k in OUT:
        assert torch.equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("name", ["m17", "mq257", "c1", "c18", "no_sigmas", "gate0", "gate_neg"])
def test_refusals_leave_the_outputs_alone(gpu_device, name):
    from spe import _lib
    rng = np.random.default_rng(0)
    # arrays large enough for every named size: the refusal must come before anything is read
    M, B, Q, C = 17, 2, 16, 18
    pts = rng.uniform(0, 100, (M, B, Q, 2)).astype(np.float32)
    probs = rng.uniform(0, 1, (M, B, Q, C)).astype(np.float32)
    sig = np.ones((M, B, Q, 2), np.float32)
    kw = {"m17": dict(M=17, Q=15, C=12), "mq257": dict(M=1, Q=257, C=12), "c1": dict(M=2, C=1), "c18": dict(M=2, C=18),
          "no_sigmas": dict(M=2, C=12, no_sigmas=True), "gate0": dict(M=2, C=12, gate=0.0),
          "gate_neg": dict(M=2, C=12, gate=-3.0)}[name]
    rc, out = call_fuse(gpu_device, pts, probs, sig, **kw)
    assert rc == SPE_E_ARG and _lib.lib().spe_last_error()
    assert all(bool((t == FILL).all()) for t in out.values())
    # the same arrays at sizes inside the limits are taken
    rc, out = call_fuse(gpu_device, pts, probs, sig, M=16, Q=16, C=17)
    assert rc == 0


# ---------------------------------------------------------------- the Python layer
def _boxes(B, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 600, (B, 2))
    wh = np.stack([rng.uniform(200, 400, B), rng.uniform(450, 700, B)], 1)
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def _pose_ensemble(M, B, Q, seed, clip):
    from spe.config import Camera
    return es.pose_ensemble(M, B, Q, seed, clip, pr.world_for(12), Camera.K)


def _check_fused(fused, pts, probs, sig, clip, solver):
    """fuse_batch's dict against the restatement with sigma_scale = the boxes' width and height."""
    clip = np.asarray(clip, np.float32)
    scale = np.stack([clip[:, 2] - clip[:, 0], clip[:, 3] - clip[:, 1]], 1)
    ref = es.fuse_batch(pts, probs, sig, scale, sigma_floor=solver.sigma_floor, gate=solver.gate)
    assert ref["min_margin"] >= 1e-6
    np.testing.assert_array_equal(fused["n_kept"].cpu().numpy(), ref["n_kept"])
    for k in ("points", "probs", "sigmas"):
        assert within_one_ulp(fused[k].cpu().numpy(), ref[k]).all(), k
    return ref


@pytest.mark.parametrize("backend", ["epnp_ransac_sigma", "epnp_ceres", "exhaustive", "epnp", "ransac_p3p_lm"])
def test_solve_batch_multi_is_the_backend_on_the_fused_arrays(gpu_device, backend):
    import torch
    from spe.solver import SigmaEnsemblePoseSolver, build_solver
    dev, M, B, Q = gpu_device, 3, 5, 30
    clip = _boxes(B, 31)
    pts, probs, sig = _pose_ensemble(M, B, Q, 32, clip)
    solver = build_solver(argparse.Namespace(solver="ensemble_sigma", backend=backend))
    assert isinstance(solver, SigmaEnsemblePoseSolver)
    lists = [[_dev(a[m], dev) for m in range(M)] for a in (pts, probs, sig)]
    dclip = _dev(clip, dev)
    kw = dict(area=[200.0] * B) if backend in ("epnp_ceres", "exhaustive") else {}
    poses = solver.solve_batch_multi(*lists, clip_bbox=dclip, **kw)
    f = poses["fused"]
    ref = _check_fused(f, pts, probs, sig, clip, solver)
    assert (ref["n_kept"][:, :11] >= 2).all()              # every label fused from two or three models
    direct = solver.backend.solve_batch(f["points"], f["probs"], f["sigmas"], **kw)
    torch.cuda.synchronize()
    assert (poses["status"] == 0).all()
    for k, v in direct.items():
        assert torch.equal(poses[k], v), k
    a, b = solver.self_assess(f["probs"], f["sigmas"], poses), solver.backend.self_assess(f["probs"], f["sigmas"], direct)
    c = solver.pose_covariance(f["probs"], f["sigmas"], poses, clip_bbox=dclip)
    d = solver.backend.pose_covariance(f["probs"], f["sigmas"], direct, clip_bbox=dclip)
    torch.cuda.synchronize()
    for x, y in ((a, b), (c, d)):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), k
    assert (c["cov_status"] == 0).all() and a["reliable"].any()
    with pytest.raises(ValueError, match="multi_sigmas"):
        solver.solve_batch_multi(lists[0], lists[1])


def test_generate_submission_with_three_sigma_models(gpu_device):
    """generate_submission(pose_cov=True) from 3 JPEG files (batch size 2, a short last batch) with three
    stand-in sigma models that return synthetic outputs for the crop boxes they are handed: each record's
    pose, pred_score and cov_status are those of the solver's own calls on the fused arrays, which are the
    restatement's for the transform's clip_bbox."""
    import io
    import torch
    from PIL import Image
    from spe.datasets import JpegDecoder
    from spe.engine import generate_submission
    from spe.solver import Multi_Mean_PoseSolver, build_solver
    dev, M, Q = gpu_device, 3, 30
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
    batches = {}

    def model_of(m):
        def model(crops, clip_bbox=None):
            clip = clip_bbox.cpu().numpy()
            key = clip.tobytes()
            if key not in batches:
                batches[key] = (clip, _pose_ensemble(M, len(clip), Q, 40 + len(batches), clip))
            pts, probs, sig = batches[key][1]
            return {"points_px": _dev(pts[m], dev), "probs": _dev(probs[m], dev), "sigmas": _dev(sig[m], dev)}
        return model

    models = [model_of(m) for m in range(M)]
    solver = build_solver(argparse.Namespace(solver="ensemble_sigma"))
    log = generate_submission(models, None, anns, files.__getitem__, solver, dev, 2, 256, decoder=dec, pose_cov=True)
    assert list(log) == names and [len(c) for c, _ in batches.values()] == [2, 1]
    i = 0
    for clip, (pts, probs, sig) in batches.values():
        dclip = _dev(clip, dev)
        f = solver.fuse_batch(*[[_dev(a[m], dev) for m in range(M)] for a in (pts, probs, sig)], clip_bbox=dclip)
        _check_fused(f, pts, probs, sig, clip, solver)
        poses = solver.backend.solve_batch(f["points"], f["probs"], f["sigmas"])
        cov = solver.backend.pose_covariance(f["probs"], f["sigmas"], poses, clip_bbox=dclip)
        torch.cuda.synchronize()
        assert (poses["status"] == 0).all() and (cov["cov_status"] == 0).all()
        for b in range(len(clip)):
            rec = log[names[i]]
            assert set(rec) == {"quat_pr", "tvec_pr", "pred_score", "cov_status"} and rec["cov_status"] == 0
            assert rec["pred_score"] == float(np.around(cov["pred_score"].cpu().numpy()[b], decimals=8)) > 0
            assert rec["tvec_pr"] == np.around(poses["tvec"][b].cpu().numpy(), decimals=6).tolist()
            assert rec["quat_pr"] == np.around(poses["quat"][b].double().cpu().numpy(), decimals=6).tolist()
            i += 1
    # a model without sigmas, and pose_cov with the unweighted ensemble, are still refused
    bare = lambda crops, clip_bbox=None: {k: v for k, v in models[0](crops, clip_bbox=clip_bbox).items() if k != "sigmas"}
    with pytest.raises(ValueError, match="sigma head"):
        generate_submission([models[0], bare], None, anns, files.__getitem__, solver, dev, 2, 256, decoder=dec)
    with pytest.raises(ValueError, match="no fusion rule for sigmas"):
        generate_submission(models, None, anns, files.__getitem__, Multi_Mean_PoseSolver(), dev, 2, 256, decoder=dec,
                            pose_cov=True)
