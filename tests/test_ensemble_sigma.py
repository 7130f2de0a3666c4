"""CPU: the sigma-weighted ensemble fusion's definition (include/spe.h spe_ensemble_fuse_sigma) as restated
in tests/ensemble_sigma_ref.py -- its properties, one constructed comparison with the REV rule
(oracle/ensemble_ref.py) -- and the host side: the exported symbol and what generate_submission hands to an
ensemble solver.  The kernel against the restatement: tests/test_gpu_ensemble_sigma.py.
"""
import types

import numpy as np
import pytest
import torch

import ensemble_ref as er
import ensemble_sigma_ref as es

C = 12


def _one(xs, sig, **kw):
    pts, probs, s = es.simple_case(xs, sig, C)
    rows, margins = es.fuse_image(pts, probs, s, **kw)
    return rows, margins


def test_one_model_is_the_identity():
    pts, probs, sig, _ = es.ensemble_inputs(1, 3, 11, C, seed=3)
    sig[0, 0, :, 0] = 1e-6                                  # below the floor on x in image 0
    o = es.fuse_batch(pts, probs, sig, sigma_floor=0.25)
    assert o["min_margin"] == np.inf                        # one measurement: no gate decision
    for b in range(3):
        meas = es.measurements(pts[:, b], probs[:, b], sig[:, b], None, 0.25)
        usable = {l: r[0] for l, r in meas.items() if r[0]["usable"]}
        assert sorted(o["labels"][b]) == sorted(usable)
        for i, l in enumerate(o["labels"][b]):
            q = usable[l]["q"]
            # (w x) / w may move x by an fp64 rounding; the float32 output is the selected point exactly
            np.testing.assert_array_equal(o["points"][b, i].astype(np.float32), pts[0, b, q])
            want = np.maximum(sig[0, b, q].astype(np.float64), 0.25)
            np.testing.assert_allclose(o["sigmas"][b, i], want, rtol=1e-15)
            assert o["probs"][b, i, l] == float(probs[0, b, q, l]) and o["n_kept"][b, i] == 1
    assert (o["sigmas"][0, :len(o["labels"][0]), 0] == 0.25).all()


def test_equal_sigmas_give_the_plain_mean():
    rng = np.random.default_rng(1)
    for n in (2, 3, 5, 9):
        xs = 500 + rng.normal(size=(n, 2)) * 0.8
        rows, _ = _one(xs, [[1.5, 1.5]] * n, gate=1e9)
        xs = xs.astype(np.float32).astype(np.float64)
        r = rows[0]
        np.testing.assert_allclose([r["x"], r["y"]], xs.mean(0), rtol=1e-14)
        for k, ax in (("sx", 0), ("sy", 1)):
            chi2 = ((xs[:, ax] - xs[:, ax].mean()) ** 2).sum() / 1.5 ** 2
            birge = max(1.0, np.sqrt(chi2 / (n - 1)))
            np.testing.assert_allclose(r[k], 1.5 / np.sqrt(n) * birge, rtol=1e-12)
    # scatter far below the sigmas: the factor is 1 exactly; far above: it widens the result
    assert _one([[10, 10], [10.01, 10]], [[2, 2]] * 2)[0][0]["sx"] == pytest.approx(2 / np.sqrt(2), rel=1e-15)
    assert _one([[10, 10], [18, 10]], [[2, 2]] * 2)[0][0]["sx"] == pytest.approx(2 / np.sqrt(2) * np.sqrt(32 / 4), rel=1e-12)


def test_two_measurements_are_never_gated():
    rows, margins = _one([[100, 100], [900, 100]], [[0.5, 0.5]] * 2)
    assert rows[0]["n_kept"] == 2 and rows[0]["kept_models"] == [0, 1] and not margins
    assert rows[0]["x"] == 500.0


def test_outlier_among_honest_measurements_is_dropped():
    rng = np.random.default_rng(2)
    for n in (3, 4, 7):
        xs = 800 + rng.normal(size=(n, 2))
        bad = int(rng.integers(n))
        xs[bad, 0] += 40.0
        rows, margins = _one(xs, [[1.0, 1.0]] * n)
        r = rows[0]
        assert r["n_pooled"] == n and r["n_kept"] == n - 1 and bad not in r["kept_models"]
        assert abs(r["x"] - 800) < 2.0 and min(margins) > 1e-6
    # the lowest model goes on a tie: two points equally far from a third on either side
    rows, _ = _one([[790, 600], [800, 600], [810, 600]], [[1.0, 1.0]] * 3)
    assert rows[0]["kept_models"] == [1, 2]


def test_permuting_the_models_keeps_the_same_measurements():
    pts, probs, sig, _ = es.ensemble_inputs(5, 4, 30, C, seed=7)
    o = es.fuse_batch(pts, probs, sig)
    perm = np.array([3, 0, 4, 2, 1])
    p = es.fuse_batch(pts[perm], probs[perm], sig[perm])
    assert (o["n_kept"] != o["n_pooled"]).any()
    for b in range(4):
        a = {l: sorted(k) for l, k in zip(o["labels"][b], o["kept"][b])}
        c = {l: sorted(int(perm[m]) for m in k) for l, k in zip(p["labels"][b], p["kept"][b])}
        assert a == c
        ia, ic = np.argsort(o["labels"][b]), np.argsort(p["labels"][b])
        np.testing.assert_allclose(o["points"][b][ia], p["points"][b][ic], rtol=1e-13)
        np.testing.assert_allclose(o["sigmas"][b][ia], p["sigmas"][b][ic], rtol=1e-10)


def test_sigma_scale_equals_prescaled_sigmas():
    # powers of two scale exactly, so both paths see the same fp64 sigmas
    pts, probs, sig, _ = es.ensemble_inputs(4, 3, 30, C, seed=9)
    scale = np.array([[256, 512], [128, 1024], [512, 256]], np.float32)
    a = es.fuse_batch(pts, probs, sig / scale[None, :, None, :], sigma_scale=scale)
    b = es.fuse_batch(pts, probs, sig)
    assert a["labels"] == b["labels"] and a["kept"] == b["kept"]
    np.testing.assert_array_equal(a["points"], b["points"])
    np.testing.assert_array_equal(a["sigmas"] * scale[:, None, :], b["sigmas"])    # leaves in the input's unit
    bad = es.fuse_batch(pts, probs, sig, sigma_scale=np.array([[256, 0], [np.nan, 2], [1, 1]], np.float32))
    assert bad["labels"][0] == [] and bad["labels"][1] == [] and bad["labels"][2] == b["labels"][2]


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_non_finite_sigma_counts_as_pooled_only(bad):
    pts, probs, sig = es.simple_case([[100, 100], [101, 100], [100, 101]], [[1, 1]] * 3, C)
    sig[1, 0, 1] = bad
    rows, _ = es.fuse_image(pts, probs, sig)
    assert rows[0]["n_pooled"] == 3 and rows[0]["n_kept"] == 2 and rows[0]["kept_models"] == [0, 2]
    sig[0, 0, 0] = sig[2, 0, 0] = bad                       # no usable measurement: not emitted
    assert es.fuse_batch(pts[:, None], probs[:, None], sig[:, None])["labels"] == [[]]
    pts[1, 0, 0] = np.nan                                   # a point that is no number is left out too
    sig[:] = 1
    assert es.fuse_image(pts, probs, sig)[0][0]["kept_models"] == [0, 2]


def test_label_of_one_model_only_and_row_order():
    pts = np.zeros((2, 3, 2), np.float32)
    probs = np.full((2, 3, C), 0.01, np.float32)
    sig = np.ones((2, 3, 2), np.float32)
    probs[:, :, C - 1] = 0.9
    for m, q, l, x in ((0, 1, 7, 70.0), (0, 2, 2, 20.0), (1, 0, 4, 40.0), (1, 1, 2, 22.0), (1, 2, 7, 71.0)):
        probs[m, q, C - 1], probs[m, q, l], pts[m, q] = 0.01, 0.8, x
    o = es.fuse_batch(pts[:, None], probs[:, None], sig[:, None])
    assert o["labels"] == [[7, 2, 4]]                       # first seen: model 0's queries, then model 1's
    np.testing.assert_array_equal(o["n_kept"][0, :4], [2, 2, 1, 0])
    assert o["points"][0, 2, 0] == 40.0 and o["sigmas"][0, 2, 0] == 1.0
    np.testing.assert_array_equal(o["probs"][0, 3], np.eye(C)[C - 1])
    assert o["probs"][0, 0, 7] == pytest.approx(0.8) and o["probs"][0, 0].sum() == o["probs"][0, 0, 7]


def test_all_background_image_gives_unused_rows():
    pts, probs, sig, _ = es.ensemble_inputs(3, 2, 11, C, seed=4)
    o = es.fuse_batch(pts, probs, sig)
    assert o["labels"][1] == [] and o["labels"][0]
    for k in ("points", "sigmas", "n_pooled", "n_kept"):
        assert not o[k][1].any()
    np.testing.assert_array_equal(o["probs"][1], np.tile(np.eye(C)[C - 1], (C - 1, 1)))


def test_honest_large_sigma_beats_the_unweighted_mean():
    """M = 3; on labels 3 and 8 model 2 is 40 px off and says so (sigma 40 px), and model 1 is 15 px off and
    says so (sigma 15 px); every other sigma is 1 px.  The sigma-weighted points stay within 3 px of the
    truth there with all three measurements kept.  The REV rule (oracle/ensemble_ref.py: the unweighted
    mean of the points closer than 3 std of their distances to the mean) ends more than 5 px away whether or
    not its filter drops the far point: it cannot tell the 1 px measurement from the 15 px one.  (With the
    other two within a pixel of each other the REV filter does drop a lone 40 px point among three -- the
    distances are about r, r, 2r and 2r > 3 std = 1.41 r -- and both rules then land within a pixel of each
    other; the graded errors are what separates them.)  On the other labels, all sigmas 1 px, the
    sigma-weighted point is within 3 px."""
    rng = np.random.default_rng(11)
    truth = rng.uniform(200, 1700, (C - 1, 2))
    pts = (truth[None] + rng.normal(size=(3, C - 1, 2))).astype(np.float32)
    sig = np.ones((3, C - 1, 2), np.float32)
    for l in (3, 8):
        pts[1, l] = (truth[l] + (15.0, -12.0)).astype(np.float32)
        sig[1, l] = 15.0
        pts[2, l] = (truth[l] + (40.0, 40.0)).astype(np.float32)
        sig[2, l] = 40.0
    probs = np.full((3, C - 1, C), 0.01, np.float32)
    probs[:, np.arange(C - 1), np.arange(C - 1)] = 0.8
    rows, _ = es.fuse_image(pts, probs, sig)
    labels, mean = er.fuse(pts, probs, C)
    assert labels == [r["label"] for r in rows] == list(range(C - 1))
    for l in range(C - 1):
        e_sigma = np.hypot(rows[l]["x"] - truth[l, 0], rows[l]["y"] - truth[l, 1])
        e_mean = np.linalg.norm(mean[l] - truth[l])
        print(l, "error of the sigma-weighted point %.3f px, of the REV rule's %.3f px" % (e_sigma, e_mean))
        assert e_sigma < 3.0
        if l in (3, 8):
            assert e_sigma < e_mean and e_mean > 5.0 and rows[l]["n_kept"] == 3


# ---------------------------------------------------------------- ABI and host logic
def test_abi_exports_ensemble_fuse_sigma():
    import os
    import re
    from conftest import REPO
    from spe import _lib
    L = _lib.lib()
    assert "spe_ensemble_fuse_sigma" in _lib.EXPORTS
    assert hasattr(L, "spe_ensemble_fuse_sigma")
    assert len(L.spe_ensemble_fuse_sigma.argtypes) == 16
    assert re.search(r"^int spe_ensemble_fuse_sigma\(", open(os.path.join(REPO, "include", "spe.h")).read(), re.M)
    assert L.spe_abi_version() == _lib.ABI_VERSION == 9


def _run(models, solver, pose_cov=False):
    """generate_submission over 5 stub files in batches of 2 on the CPU (stub decoder and transform, in
    the style of tests/test_submission_front.py)."""
    from spe.engine import generate_submission
    H, W = 4, 6

    def decoder(data, offsets, sizes):
        raw = data.numpy().tobytes()
        frames = torch.stack([torch.full((H, W), int(raw[o:o + n]), dtype=torch.uint8)
                              for o, n in zip(offsets.tolist(), sizes.tolist())])
        return {"frames": frames, "status": torch.zeros(len(frames), dtype=torch.int32)}

    def transform(frames, bbox, crops=False, images=True):
        bb = torch.as_tensor(bbox, dtype=torch.float32)
        return {"crops": frames, "clip_bbox": bb, "status": torch.zeros(len(bb), dtype=torch.int32)}

    files = {f"f{i}.jpg": str(10 * i + 3).encode() for i in range(5)}
    anns = {f: [[float(i), 2.0, 30.0 + i, 50.0, 0.9]] for i, f in enumerate(files)}
    return generate_submission(models, None, anns, files.__getitem__, solver, torch.device("cpu"), 2, 8,
                               decoder=decoder, transform=transform, pose_cov=pose_cov), anns


def _model(k, with_sigma=True):
    def forward(crops, clip_bbox=None):
        v = crops.reshape(crops.shape[0], -1).float().mean(1) + k
        o = {"points_px": v[:, None, None].expand(-1, 11, 2), "probs": (v / 100)[:, None, None].expand(-1, 11, 12)}
        if with_sigma:
            o["sigmas"] = (v * 2)[:, None, None].expand(-1, 11, 2)
        return o
    return forward


def _poses(v):
    B = v.shape[0]
    return {"quat": v[:, None].float().expand(B, 4), "tvec": v[:, None].double().expand(B, 3),
            "status": torch.zeros(B, dtype=torch.int32)}


def _sigma_stub(mode=1):
    from spe.solver import SigmaEnsemblePoseSolver

    class Stub(SigmaEnsemblePoseSolver):
        def __init__(self):
            self.backend = types.SimpleNamespace(mode=mode)
            self.calls, self.cov_calls = [], []

        def solve_batch_multi(self, multi_points_px, multi_probs, multi_sigmas=None, clip_bbox=None, **kw):
            assert not kw
            self.calls.append((multi_points_px, multi_probs, multi_sigmas, clip_bbox))
            p = _poses(torch.stack(list(multi_points_px)).mean(0)[:, 0, 0])
            p["fused"] = {"probs": multi_probs[0] + 5, "sigmas": multi_sigmas[-1] + 7}
            return p

        def pose_covariance(self, probs, sigmas, poses, clip_bbox=None):
            self.cov_calls.append((probs, sigmas, poses, clip_bbox))
            return {"pred_score": sigmas[:, 0, 0], "cov_status": torch.zeros(len(probs), dtype=torch.int32)}

    return Stub()


def test_generate_submission_hands_sigmas_and_boxes_to_a_sigma_ensemble():
    s = _sigma_stub()
    log, anns = _run([_model(0), _model(1), _model(2)], s, pose_cov=True)
    assert [c[3].shape[0] for c in s.calls] == [2, 2, 1]
    boxes = np.asarray([a[0][:4] for a in anns.values()], np.float32)
    np.testing.assert_array_equal(torch.cat([c[3] for c in s.calls]).numpy(), boxes)
    for pts, probs, sigmas, clip in s.calls:
        assert len(pts) == len(probs) == len(sigmas) == 3
        for k in range(3):                                  # model k's own sigmas, in the models' order
            assert torch.equal(sigmas[k], pts[k] * 2) and torch.equal(probs[k], pts[k][..., :1].expand(-1, -1, 12) / 100)
        assert torch.equal(pts[2], pts[0] + 2)
    # pose_cov reads the fused probs and sigmas with the batch's boxes
    assert len(s.cov_calls) == 3
    for (pts, probs, sigmas, clip), (cp, cs, poses, cclip) in zip(s.calls, s.cov_calls):
        assert torch.equal(cp, probs[0] + 5) and torch.equal(cs, sigmas[-1] + 7) and torch.equal(cclip, clip)
        assert "fused" in poses
    assert list(log) == list(anns)
    assert all(set(r) == {"quat_pr", "tvec_pr", "pred_score", "cov_status"} for r in log.values())
    assert log["f1.jpg"]["tvec_pr"][0] == 14.0 and log["f1.jpg"]["pred_score"] == (13.0 + 2) * 2 + 7
    with pytest.raises(ValueError, match="sigma head"):
        _run([_model(0), _model(1, with_sigma=False)], _sigma_stub())
    from spe import _lib
    with pytest.raises(ValueError, match="EPnPCeresSolver"):
        _run([_model(0), _model(1)], _sigma_stub(mode=_lib.SPE_PNP_EPNP_CERES))


def test_generate_submission_keeps_the_two_argument_call_for_other_ensembles():
    class Other:
        def __init__(self):
            self.calls = []

        def solve_batch_multi(self, multi_points, multi_probs):
            self.calls.append((len(multi_points), len(multi_probs)))
            return _poses(torch.stack(list(multi_points)).mean(0)[:, 0, 0])

    s = Other()
    log, anns = _run([_model(0), _model(4)], s)
    assert s.calls == [(2, 2)] * 3 and log["f0.jpg"]["tvec_pr"][0] == 5.0
    with pytest.raises(ValueError, match="no fusion rule for sigmas"):
        _run([_model(0), _model(4)], Other(), pose_cov=True)


def test_build_solver_wraps_the_backend():
    import argparse
    from spe import _lib
    from spe.solver import ExhaustivePoseSolver, SigmaEnsemblePoseSolver, SimplePoseSolverSigma, build_solver
    s = build_solver(argparse.Namespace(solver="ensemble_sigma"))
    assert isinstance(s, SigmaEnsemblePoseSolver) and isinstance(s.backend, SimplePoseSolverSigma)
    assert s.gate == 3.0 and s.sigma_floor == 1e-3 and s.mode == _lib.SPE_PNP_EPNP_RANSAC_SIGMA
    s = build_solver(argparse.Namespace(solver="ensemble_sigma", backend="exhaustive", topk=4, gate=2.5, sigma_floor=0.01))
    assert isinstance(s.backend, ExhaustivePoseSolver) and s.backend.topk == 4 and (s.gate, s.sigma_floor) == (2.5, 0.01)
    with pytest.raises(ValueError):
        SigmaEnsemblePoseSolver(gate=0.0)
    with pytest.raises(ValueError, match="multi_sigmas"):
        s.solve_batch_multi([torch.zeros(1, 2, 2)], [torch.zeros(1, 2, 12)])
