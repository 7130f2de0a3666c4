"""GPU: what the host code runs after the model -- the solve, the score, the self-assessment, the pose
covariance and the calibration / landmark accumulators -- as a sequence of calls, for each of its four callers:
PosePipeline.run, evaluate, evaluate_rtdetr and generate_submission.

A recorder stands in for the solver.  It forwards every call to a real solver and logs, per call, the method's
name, the sorted names of the keywords it was called with, whatever their values (the pipeline names stream= in
every call, None in its serial mode; the three loops never do, so a solver object without the keyword serves them)
and which of sigma_gain / sigma_scale / area / repro_per_image / stream were among them; the streams themselves
are kept too.  Calibration.update and LandmarkReconstruction.update log into the same list; the calibration's entry also says whether the covariance it was handed came from a pose_covariance
call without a gain (the accumulator applies its own).  The expected sequences are literals: they describe
what each caller does per batch and were written down before the callers shared any code.

Shapes are the smallest the callers take: B = 2 (3 files at batch size 2 for generate_submission, so a short
last batch occurs), a 2 + 2 layer DETR with a sigma head at 128 x 128 and the r18 RT-DETR at 128 x 128, random
weights.  Poses need not be solved for a call sequence, so nothing numeric is compared here (the per-feature
files do that).
"""
import argparse
import io

import numpy as np
import pytest
import torch

from lens_ref import DIST
from spe import _lib

pytestmark = pytest.mark.gpu

B, S = 2, 128
FLAGS = ("sigma_gain", "sigma_scale", "area", "repro_per_image", "stream")
COV_KEYS = {"pose_cov", "sigma_rot", "sigma_t", "pred_score", "cov_status"}


def call(name, *kws):
    """The log entry of one call with the keywords `kws`."""
    return (name, tuple(sorted(kws)), tuple(k in kws for k in FLAGS))


def _entry(name, kw):
    return call(name, *kw)


class Recorder:
    """A solver object that forwards to `solver` and logs its calls into `log`."""

    def __init__(self, solver, log):
        self._s, self.log, self.gain_free, self.streams = solver, log, [], []

    __class__ = property(lambda self: type(self._s))          # isinstance() sees the real solver's class

    def __getattr__(self, k):
        return getattr(self._s, k)

    def _logged(self, name, args, kw):
        self.log.append(_entry(name, kw))
        self.streams.append(kw.get("stream"))
        return getattr(self._s, name)(*args, **kw)

    def solve_batch(self, *a, **kw):
        return self._logged("solve_batch", a, kw)

    def solve_batch_multi(self, *a, **kw):
        return self._logged("solve_batch_multi", a, kw)

    def self_assess(self, *a, **kw):
        return self._logged("self_assess", a, kw)

    def pose_covariance(self, *a, **kw):
        cov = self._logged("pose_covariance", a, kw)
        if "sigma_gain" not in kw:
            self.gain_free.append(cov["pose_cov"])
        return cov


class NoGainRecorder(Recorder):
    """A solver object from before sigma_gain: its pose_covariance does not know the keyword."""

    def pose_covariance(self, probs, sigmas, poses, clip_bbox=None, **stream):
        if stream.keys() - {"stream"}:
            raise TypeError(f"pose_covariance() got an unexpected keyword argument {sorted(stream.keys() - {'stream'})[0]!r}")
        cov = self._logged("pose_covariance", (probs, sigmas, poses), dict(clip_bbox=clip_bbox, **stream))
        self.gain_free.append(cov["pose_cov"])
        return cov


@pytest.fixture
def log(monkeypatch):
    """The call log; the two accumulators' update() write into it too."""
    from spe.calibration import Calibration
    from spe.landmarks import LandmarkReconstruction
    entries = []
    cal_update, lm_update = Calibration.update, LandmarkReconstruction.update

    def cal(self, points_px, probs, sigmas, poses, cov, *a, **kw):
        free = any(cov["pose_cov"] is t for t in getattr(self.solver, "gain_free", []))
        entries.append(_entry("Calibration.update", kw) + (free,))
        return cal_update(self, points_px, probs, sigmas, poses, cov, *a, **kw)

    def lm(self, *a, **kw):
        entries.append(_entry("LandmarkReconstruction.update", kw))
        return lm_update(self, *a, **kw)

    monkeypatch.setattr(Calibration, "update", cal)
    monkeypatch.setattr(LandmarkReconstruction, "update", lm)
    return entries


def cal_update(*kws):
    return call("Calibration.update", *kws) + (True,)


def _solver(name="epnp_ransac_sigma", lens=False, **kw):
    from spe.solver import build_solver
    return build_solver(argparse.Namespace(solver=name, input_size=S, **(dict(dist=list(DIST)) if lens else {}), **kw))


@pytest.fixture(scope="module")
def detr(gpu_device):
    """(cfg, model): the small DETR with a sigma head."""
    from spe.config import SpeConfig
    from spe.models import DETR
    from spe.synthetic import random_weights
    cfg = SpeConfig(input_size=S, num_queries=11, enc_layers=2, dec_layers=2, sigma_head=True)
    m = DETR(cfg, dtype="bf16")
    m.load_state_dict(random_weights(cfg, 3))
    return cfg, m


@pytest.fixture(scope="module")
def rtdetr(gpu_device):
    from spe.rtdetr import RTDETR
    from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights
    cfg = RtdetrConfig(depth=18, input_size=S)
    m = RTDETR(cfg, dtype="bf16")
    m.load_state_dict(random_rtdetr_weights(cfg, 0))
    return m


@pytest.fixture(scope="module")
def batch(detr):
    """One synthetic batch (numpy: images, clip_bbox, quat, tvec) and the evaluate loops' loader and ground truth."""
    from spe.synthetic import synthetic_batch
    b = synthetic_batch(detr[0], B, 31)
    names = [f"img{i}.jpg" for i in range(B)]
    gt = {n: {"quat": b["quat"][i].tolist(), "tvec": b["tvec"][i].tolist(), "area": 300.0 + 40 * i}
          for i, n in enumerate(names)}
    loader = [(torch.from_numpy(b["images"]), [{"filename": n, "clip_bbox": torch.as_tensor(b["clip_bbox"][i])}
                                               for i, n in enumerate(names)])]
    return b, loader, gt


# ---------------------------------------------------------------- PosePipeline

SOLVE_ASSESS = [call("solve_batch"), call("self_assess")]                           # the loops
PIPE = [call("solve_batch", "stream"), call("self_assess", "stream")]               # the pipeline, every mode
PIPE_COV = [call("pose_covariance", "clip_bbox", "stream")]
PIPE_COV2 = [call("pose_covariance", "clip_bbox", "sigma_gain", "stream")]
PIPE_CAL = [cal_update("clip_bbox", "stream")]
PIPELINE = {
    "plain": (dict(), {}, PIPE),
    "overlap": (dict(), dict(overlap=True), PIPE),
    "overlap_decode": (dict(), dict(overlap_decode=True), PIPE),
    "no_assess": (dict(), dict(self_assess=False), PIPE[:1]),
    "lens": (dict(lens=True), {}, [call("solve_batch", "sigma_scale", "stream"), PIPE[1]]),
    "lens_overlap": (dict(lens=True), dict(overlap=True), [call("solve_batch", "sigma_scale", "stream"), PIPE[1]]),
    "ceres": (dict(name="epnp_ceres"), {}, [call("solve_batch", "repro_per_image", "stream"), PIPE[1]]),
    "ceres_overlap_decode": (dict(name="epnp_ceres"), dict(overlap_decode=True),
                             [call("solve_batch", "repro_per_image", "stream"), PIPE[1]]),
    "cov_gain1": (dict(), dict(pose_cov=True), PIPE + PIPE_COV),
    "cov_gain2": (dict(), dict(pose_cov=True, sigma_gain=2.0), PIPE + PIPE_COV2),
    "cov_gain2_overlap": (dict(), dict(pose_cov=True, sigma_gain=2.0, overlap=True), PIPE + PIPE_COV2),
    "cal_gain1": (dict(), dict(calibration=1.0), PIPE + PIPE_COV + PIPE_CAL),
    "cal_gain2": (dict(), dict(calibration=2.0, sigma_gain=2.0), PIPE + PIPE_COV2 + PIPE_COV + PIPE_CAL),
    "cal_gain2_overlap_decode": (dict(), dict(calibration=2.0, sigma_gain=2.0, overlap_decode=True),
                                 PIPE + PIPE_COV2 + PIPE_COV + PIPE_CAL),
}


def _run_pipeline(dev, model, solver, b, kw):
    from spe.pipeline import PosePipeline
    p = PosePipeline(model, solver, B, device=dev, **kw)
    area = dict(area=[300.0, 340.0]) if solver.mode == _lib.SPE_PNP_EPNP_CERES else {}
    p.load(torch.from_numpy(b["images"]).to(dev), torch.from_numpy(b["clip_bbox"]).float().to(dev),
           torch.from_numpy(b["quat"]).to(dev), torch.from_numpy(b["tvec"]).to(dev), **area)
    out = p.run()
    p.wait(out)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", sorted(PIPELINE))
def test_pipeline_step(gpu_device, detr, batch, log, case):
    """One run() of the pipeline; its dict is flat, the covariance's keys beside the others."""
    from spe.calibration import Calibration
    skw, pkw, want = PIPELINE[case]
    pkw = dict(pkw)
    solver = Recorder(_solver(**skw), log)
    if "calibration" in pkw:
        pkw["calibration"] = Calibration(sigma_gain=pkw["calibration"], solver=solver)
    out = _run_pipeline(gpu_device, detr[1], solver, batch[0], pkw)
    assert log == want
    assert all(s is out.get("stream") for s in solver.streams)      # None in the serial modes, else the solver stream
    keys = {"forward", "poses", "s_t", "s_q"} | ({"assess"} if pkw.get("self_assess", True) else set())
    if pkw.get("pose_cov") or "calibration" in pkw:
        keys |= COV_KEYS
    if "calibration" in pkw:
        keys |= {"calibration"}
    if any(pkw.get(k) for k in ("overlap", "overlap_decode")):
        keys |= {"stream"}
    assert set(out) == keys
    if "lens" in skw:
        assert {"points_ideal", "sigmas_ideal", "lens_status"} <= set(out["poses"])


def test_pipeline_with_a_solver_from_before_sigma_gain(gpu_device, detr, batch, log):
    """At gain 1 the keyword is left out: a solver object whose pose_covariance lacks it keeps working, also
    under a calibration; at another gain it is passed."""
    from spe.calibration import Calibration
    solver = NoGainRecorder(_solver(), log)
    out = _run_pipeline(gpu_device, detr[1], solver, batch[0], dict(pose_cov=True))
    assert COV_KEYS <= set(out)
    _run_pipeline(gpu_device, detr[1], solver, batch[0], dict(calibration=Calibration(solver=solver)))
    assert log == PIPE + PIPE_COV + PIPE + PIPE_COV + PIPE_CAL
    with pytest.raises(TypeError, match="sigma_gain"):
        _run_pipeline(gpu_device, detr[1], solver, batch[0], dict(pose_cov=True, sigma_gain=2.0))


# ---------------------------------------------------------------- evaluate

EVALUATE = {
    "plain": (dict(), {}, SOLVE_ASSESS),
    "lens": (dict(lens=True), {}, [call("solve_batch", "sigma_scale"), call("self_assess")]),
    "ceres": (dict(name="epnp_ceres"), {}, [call("solve_batch", "area"), call("self_assess")]),
    "cal_gain1": (dict(), dict(calibration=True),
                  SOLVE_ASSESS + [call("pose_covariance", "clip_bbox"), cal_update("clip_bbox")]),
    "cal_gain2": (dict(), dict(calibration=True, sigma_gain=2.0),
                  SOLVE_ASSESS + [call("pose_covariance", "clip_bbox"), cal_update("clip_bbox")]),
    "landmarks": (dict(), dict(landmarks=True),
                  SOLVE_ASSESS + [call("LandmarkReconstruction.update", "sigma_scale")]),
    "landmarks_cal": (dict(), dict(landmarks=True, calibration=True),
                      SOLVE_ASSESS + [call("LandmarkReconstruction.update", "sigma_scale"),
                                             call("pose_covariance", "clip_bbox"), cal_update("clip_bbox")]),
}


def _landmarks(kw):
    from spe.landmarks import LandmarkReconstruction
    kw = dict(kw)
    if kw.get("landmarks"):
        kw["landmarks"] = LandmarkReconstruction(num_landmarks=11)
    return kw


@pytest.mark.parametrize("case", sorted(EVALUATE))
def test_evaluate_batch(gpu_device, detr, batch, log, case):
    from spe.engine import evaluate
    skw, ekw, want = EVALUATE[case]
    solver = Recorder(_solver(**skw), log)
    stats, ev = evaluate(detr[1], None, None, batch[1], batch[2], solver, gpu_device, **_landmarks(ekw))
    assert log == want
    assert all({"sigma", "mean_sigma", "reliable"} <= set(r) for r in ev.log.values()) and len(ev.log) == B
    assert ("calibration" in stats) == bool(ekw.get("calibration"))
    if ekw.get("sigma_gain"):
        assert stats["calibration"]["gain_in_force"] == ekw["sigma_gain"]


def test_evaluate_without_sigmas_assesses_nothing(gpu_device, detr, batch, log):
    """self_assess runs whenever the model has sigmas, and only then; no sigma scale goes to a lens solver."""
    from spe.engine import evaluate
    m = detr[1]

    def model(samples, clip_bbox=None):
        return {k: v for k, v in m(samples, clip_bbox=clip_bbox).items() if k != "sigmas"}

    for lens in (False, True):
        del log[:]
        _, ev = evaluate(model, None, None, batch[1], batch[2], Recorder(_solver("ransac_p3p_lm", lens=lens), log), gpu_device)
        assert log == [call("solve_batch")]
        assert not any("reliable" in r or "sigma" in r for r in ev.log.values())


def test_evaluate_with_a_solver_from_before_sigma_gain(gpu_device, detr, batch, log):
    from spe.engine import evaluate
    solver = NoGainRecorder(_solver(), log)
    stats, _ = evaluate(detr[1], None, None, batch[1], batch[2], solver, gpu_device, calibration=True, sigma_gain=2.0)
    assert stats["calibration"]["gain_in_force"] == 2.0
    assert log == SOLVE_ASSESS + [call("pose_covariance", "clip_bbox"), cal_update("clip_bbox")]


# ---------------------------------------------------------------- evaluate_rtdetr

EVALUATE_RTDETR = {
    "plain": (dict(), {}, [call("solve_batch")]),
    "lens": (dict(lens=True), {}, [call("solve_batch", "sigma_scale")]),
    "cov_gain1": (dict(), dict(pose_cov=True), [call("solve_batch"), call("pose_covariance", "clip_bbox")]),
    "cov_gain2": (dict(), dict(pose_cov=True, sigma_gain=2.0),
                  [call("solve_batch"), call("pose_covariance", "clip_bbox", "sigma_gain")]),
    "cal_gain1": (dict(), dict(calibration=True),
                  [call("solve_batch"), call("pose_covariance", "clip_bbox"), cal_update("clip_bbox")]),
    "cal_gain2": (dict(), dict(calibration=True, sigma_gain=2.0),
                  [call("solve_batch"), call("pose_covariance", "clip_bbox"), cal_update("clip_bbox")]),
    "cov_cal_gain1": (dict(), dict(pose_cov=True, calibration=True),
                      [call("solve_batch"), call("pose_covariance", "clip_bbox"), cal_update("clip_bbox")]),
    "cov_cal_gain2": (dict(), dict(pose_cov=True, calibration=True, sigma_gain=2.0),
                      [call("solve_batch"), call("pose_covariance", "clip_bbox", "sigma_gain"),
                       call("pose_covariance", "clip_bbox"), cal_update("clip_bbox")]),
    "landmarks": (dict(), dict(landmarks=True),
                  [call("solve_batch"), call("LandmarkReconstruction.update", "sigma_scale")]),
    "lens_cov_landmarks": (dict(lens=True), dict(pose_cov=True, landmarks=True),
                           [call("solve_batch", "sigma_scale"), call("LandmarkReconstruction.update", "sigma_scale"),
                            call("pose_covariance", "clip_bbox")]),
}


@pytest.mark.parametrize("case", sorted(EVALUATE_RTDETR))
def test_evaluate_rtdetr_batch(gpu_device, rtdetr, batch, log, case):
    """The RT-DETR loop never self-assesses: its records have no assess fields."""
    from spe.engine import evaluate_rtdetr
    skw, ekw, want = EVALUATE_RTDETR[case]
    solver = Recorder(_solver(**skw), log)
    stats, ev = evaluate_rtdetr(rtdetr, None, None, batch[1], batch[2], solver, gpu_device, **_landmarks(ekw))
    assert log == want
    for r in ev.log.values():
        assert {"sigma", "aux_points_0", "aux_points_1", "aux_points_2"} <= set(r)
        assert "reliable" not in r and "mean_sigma" not in r
        assert ("pred_score" in r and "cov_status" in r) == bool(ekw.get("pose_cov"))
    assert ("calibration" in stats) == bool(ekw.get("calibration"))


def test_evaluate_rtdetr_with_a_solver_from_before_sigma_gain(gpu_device, rtdetr, batch, log):
    from spe.engine import evaluate_rtdetr
    solver = NoGainRecorder(_solver(), log)
    _, ev = evaluate_rtdetr(rtdetr, None, None, batch[1], batch[2], solver, gpu_device, pose_cov=True, calibration=True)
    assert log == [call("solve_batch"), call("pose_covariance", "clip_bbox"), cal_update("clip_bbox")]
    assert all("pred_score" in r for r in ev.log.values())


# ---------------------------------------------------------------- generate_submission

@pytest.fixture(scope="module")
def submission(gpu_device):
    """3 small gray JPEG files, their boxes and a decoder of their size."""
    from PIL import Image
    from spe.datasets import JpegDecoder
    H, W = 240, 320
    yy, xx = np.mgrid[0:H, 0:W]
    files = {}
    for i, n in enumerate(["img3.jpg", "img1.jpg", "img2.jpg"]):
        bio = io.BytesIO()
        Image.fromarray(((xx * (i + 2) + yy * 3) % 256).astype(np.uint8)).save(bio, "JPEG", quality=60)
        files[n] = bio.getvalue()
    boxes = [[60.0, 30.0, 200.0, 170.0], [-20.5, 40.0, 150.0, 200.0], [120.2, 60.9, 300.4, 180.1]]
    anns = {n: [b + [0.9]] for n, b in zip(files, boxes)}
    return files, anns, JpegDecoder(H, W, max_bytes=max(map(len, files.values())))


SUBMISSION = {
    "plain": (dict(), {}, [call("solve_batch")]),
    "lens": (dict(lens=True), {}, [call("solve_batch", "sigma_scale")]),
    "cov_gain1": (dict(), dict(pose_cov=True), [call("solve_batch"), call("pose_covariance", "clip_bbox")]),
    "cov_gain2": (dict(lens=True), dict(pose_cov=True, sigma_gain=2.0),
                  [call("solve_batch", "sigma_scale"), call("pose_covariance", "clip_bbox", "sigma_gain")]),
}


@pytest.mark.parametrize("case", sorted(SUBMISSION))
def test_generate_submission_batches(gpu_device, rtdetr, submission, log, case):
    """Two batches (2 + 1 files), each the same sequence."""
    from spe.engine import generate_submission
    files, anns, dec = submission
    skw, gkw, want = SUBMISSION[case]
    solver = Recorder(_solver(**skw), log)
    out = generate_submission(rtdetr, None, anns, files.__getitem__, solver, gpu_device, 2, S, decoder=dec, **gkw)
    assert log == 2 * want and list(out) == list(files)
    fields = {"quat_pr", "tvec_pr"} | ({"pred_score", "cov_status"} if gkw.get("pose_cov") else set())
    assert all(set(r) == fields for r in out.values())


def test_generate_submission_ensemble_and_refusals(gpu_device, rtdetr, submission, log):
    """A list of models with the sigma ensemble: the fused solve, then the covariance of the fused set; the
    Ceres solver is refused before anything runs."""
    from spe.engine import generate_submission
    from spe.solver import SigmaEnsemblePoseSolver
    files, anns, dec = submission
    solver = Recorder(SigmaEnsemblePoseSolver(_solver()), log)
    out = generate_submission([rtdetr, rtdetr], None, anns, files.__getitem__, solver, gpu_device, 2, S, decoder=dec,
                              pose_cov=True, sigma_gain=2.0)
    assert log == 2 * [call("solve_batch_multi", "clip_bbox"), call("pose_covariance", "clip_bbox", "sigma_gain")]
    assert all(set(r) == {"quat_pr", "tvec_pr", "pred_score", "cov_status"} for r in out.values())
    del log[:]
    with pytest.raises(ValueError, match="EPnPCeresSolver takes one threshold per image"):
        generate_submission(rtdetr, None, anns, files.__getitem__, Recorder(_solver("epnp_ceres"), log), gpu_device, 2, S,
                            decoder=dec)
    assert log == []
