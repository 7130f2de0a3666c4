"""What runs after the model, in one place: PosePipeline, evaluate, evaluate_rtdetr and generate_submission all
go through PostStage.  A new post-model step is added here, once.

Per batch, in this order, each step one launch (or none):
    the lens's sigma scale  a solver with a lens maps the model's crop-normalised sigmas in pixels: the crop's size
    solve_batch             with the per-image thresholds (area= / repro_per_image=) of the solvers that take them
    device_speed_score      with a ground truth
    self_assess             when asked for and the model has sigmas
    landmarks.update        a spe.landmarks.LandmarkReconstruction
    pose_covariance         when asked for, the sigmas times sigma_gain
    calibration.update      a spe.calibration.Calibration, always on the covariance at gain 1
Nothing here synchronises with the host, and everything but the landmark step is issued on `stream` when one is
given (None, or none: the current one), the small torch ops that build the sigma scale included: a step can be
captured into a HIP graph.  The landmark step has no stream argument and runs on the current stream.
"""
from __future__ import annotations

from collections import namedtuple

from .solver import sigma_scale_of
from .speed_eval import device_speed_score

# s_t / s_q: None without a ground truth; assess / cov / records: None unless asked for
Post = namedtuple("Post", "poses s_t s_q assess cov records")


class PostStage:
    """solver: any solver object of spe.solver.  self_assess, pose_cov: run those steps (a model without sigmas is
    never assessed; its covariance is the caller's error to raise).  sigma_gain: the calibration factor on the
    sigmas the covariance reads; the keyword is left out at 1.0, so a solver object whose pose_covariance lacks
    it keeps working.  calibration / landmarks: the accumulators, None: no such step.  score: what scores the
    poses (the evaluate loops hand in their module's, which a test without a device replaces)."""

    def __init__(self, solver, self_assess=False, pose_cov=False, sigma_gain=1.0, calibration=None, landmarks=None,
                 score=device_speed_score):
        self.solver, self.self_assess, self.pose_cov, self.score = solver, self_assess, pose_cov, score
        self.sigma_gain = float(sigma_gain)
        self.calibration, self.landmarks = calibration, landmarks

    def __call__(self, fo, clip, q_gt=None, t_gt=None, area=None, repro_per_image=None, poses=None, **on):
        """fo: a forward's output dict (points_px, probs and, with a sigma head, sigmas); clip: the batch's
        clip_bbox [B,4]; q_gt / t_gt: the ground truth, device fp64.  poses: a solve already done (an ensemble's
        solve_batch_multi over fo's fused arrays), the solve is then skipped.  on: stream=, or nothing -- it goes
        to every step as given, so a loop that names no stream also works with solver objects that take none.
        -> Post."""
        solver, sig = self.solver, fo.get("sigmas")
        if poses is None:
            kw = dict(on)
            if sig is not None and getattr(solver, "lens", None) is not None:
                kw["sigma_scale"] = sigma_scale_of(clip, sig.device, on.get("stream"))
            if area is not None:
                kw["area"] = area
            if repro_per_image is not None:
                kw["repro_per_image"] = repro_per_image
            poses = solver.solve_batch(fo["points_px"], fo["probs"], sig, **kw)
        s_t = s_q = assess = cov = records = None
        if q_gt is not None:
            s_t, s_q = self.score(poses["quat"], poses["tvec"], q_gt, t_gt, **on)
        if self.self_assess and sig is not None:
            assess = solver.self_assess(fo["probs"], sig, poses, **on)
        if self.landmarks is not None:
            # the model's sigmas are crop-normalised like its points: the crop's size is their scale
            self.landmarks.update(fo["points_px"], fo["probs"], sig, q_gt, t_gt,
                                  sigma_scale=sigma_scale_of(clip, sig.device) if sig is not None else None)
        if self.pose_cov:
            gain = {} if self.sigma_gain == 1.0 else {"sigma_gain": self.sigma_gain}
            cov = solver.pose_covariance(fo["probs"], sig, poses, clip_bbox=clip, **on, **gain)
        if self.calibration is not None:
            # the accumulator applies its own gain, to the covariance at gain 1
            cov1 = cov if cov is not None and self.sigma_gain == 1.0 else \
                solver.pose_covariance(fo["probs"], sig, poses, clip_bbox=clip, **on)
            records = self.calibration.update(fo["points_px"], fo["probs"], sig, poses, cov1, q_gt, t_gt, s_t, s_q,
                                              clip_bbox=clip, **on)
        return Post(poses, s_t, s_q, assess, cov, records)
