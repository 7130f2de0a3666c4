"""Pose solvers with the reference's interface (REV/utils/speed_eval.py:21-242,
UNC/utils/speed_eval.py:322-420, UNC/utils/speed_eval_ceres.py:43-169), executed by the
batched HIP solver kernel (csrc/pnp.hip) through spe_pnp_batch.

    solver = build_solver(args)                 # args.repro (20), args.solver
    quat, tvec = solver(points, logits)         # one image, numpy, like the reference
    poses = solver.solve_batch(points_px, probs) # whole batch on device (hot path)

A camera with lens distortion: every solver class takes lens=LensModel(K, dist) (build_solver: args.dist)
and then undistorts its keypoints, and their sigmas, on the device (spe_undistort_points) before the
unchanged solver kernel runs on the ideal points.

Failures raise exactly what the reference raises so SpeedEval.update maps them to a zero
pose: IndexError when no foreground label survives, SolverError (the cv2.error stand-in)
when OpenCV would assert (fewer than 4 correspondences) or leave its output undefined.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .config import Camera, LensModel, load_world

MODES = {"epnp": _lib.SPE_PNP_EPNP, "ransac_p3p_lm": _lib.SPE_PNP_RANSAC_P3P_LM,
         "epnp_ransac_sigma": _lib.SPE_PNP_EPNP_RANSAC_SIGMA, "epnp_lm": _lib.SPE_PNP_EPNP_LM,
         "epnp_ceres": _lib.SPE_PNP_EPNP_CERES}


class SolverError(RuntimeError):
    """Raised where the reference's cv2 call raises cv2.error."""


def sigma_scale_of(clip_bbox, device, stream=None):
    """clip_bbox [B,4] (x1, y1, x2, y2) -> [B,2] fp32, the crop's width and height: the pixels per unit of
    a crop-normalised sigma, per axis (the factor PostProcess applies to the points).  Made on the stream
    the kernels read it on."""
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        cb = clip_bbox.to(device=device, dtype=torch.float32)
        return torch.stack((cb[:, 2] - cb[:, 0], cb[:, 3] - cb[:, 1]), 1).contiguous()


class PoseSolver:
    """Holds the 11 world landmarks (REV/utils/speed_eval.py:28-39) and camera K.  lens (a
    spe.config.LensModel, None: a pinhole camera): its K replaces Camera.K, and solve_batch first maps
    the points and sigmas to the ideal image (undistort).  world (spe.config.load_world: an [L,3] array, a
    world_points.json-style file or a spe.landmarks.LandmarkModel; None: the packaged SPEED table): the
    landmarks every entry of this solver reads."""

    def __init__(self, mode=_lib.SPE_PNP_RANSAC_P3P_LM, repro=20.0, ransac_iters=100, confidence=0.99, lens=None,
                 world=None):
        self.W_Pt = load_world(world)
        self._own_world = world is not None
        self.K = Camera.K.copy()
        self.mode = mode
        self.reprojectionError = float(repro)
        self.ransac_iters = int(ransac_iters)
        self.confidence = float(confidence)
        self._dev = {}
        self.lens = None
        if lens is not None:
            self.set_lens(lens)

    def set_lens(self, lens):
        """Installs a LensModel: the ideal points are pixels of its K, which the solver then uses."""
        self.lens = lens
        self.K = np.array(lens.K)
        self._dev = {}
        self._lens_dist = {}
        self._lens_buf = {}

    def set_world(self, world):
        """Installs another landmark table (load_world); the device constants are made again."""
        self.W_Pt = load_world(world)
        self._own_world = world is not None
        self._dev = {}

    def _check_world(self, C):
        """A table given by the caller must cover the model's landmark classes (the kernels read C - 1 rows)."""
        if self._own_world and C - 1 > self.W_Pt.shape[0]:
            raise ValueError(f"solve_batch: {C} classes need {C - 1} landmarks, the solver's table holds "
                             f"{self.W_Pt.shape[0]}")

    def undistort(self, points_px, sigmas=None, sigma_scale=None, stream=None):
        """The lens step (include/spe.h spe_undistort_points), one launch: points_px [N,Q,2] distorted
        pixels (+ sigmas [N,Q,2], sigma_scale [N,2] pixels per sigma unit, None: the sigmas are pixels)
        -> dict of device tensors points_ideal [N,Q,2], sigmas_ideal [N,Q,2] (None without sigmas) and
        lens_status [N,Q] u8 (1: the iteration left the model's domain, the point and its sigma are
        returned unchanged).  The outputs are buffers the solver keeps per (device, shape): the next call
        with the same shape overwrites them, clone what must outlive it."""
        N, Q = points_px.shape[0], points_px.shape[1]
        dev = points_px.device
        Kd, _ = self._consts(dev)
        if str(dev) not in self._lens_dist:
            self._lens_dist[str(dev)] = torch.tensor(self.lens.dist.tolist(), dtype=torch.float64, device=dev)
        key = (str(dev), N, Q, sigmas is not None)
        if key not in self._lens_buf:
            self._lens_buf[key] = dict(points_ideal=torch.empty(N, Q, 2, device=dev),
                                       sigmas_ideal=torch.empty(N, Q, 2, device=dev) if sigmas is not None else None,
                                       lens_status=torch.empty(N, Q, dtype=torch.uint8, device=dev))
        o = dict(self._lens_buf[key])
        ins = [t.float().contiguous() if t is not None else None for t in (points_px, sigmas, sigma_scale)]
        _lib.check(_lib.lib().spe_undistort_points(
            _lib.stream_ptr(stream), _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), N, Q, _lib.ptr(Kd),
            _lib.ptr(self._lens_dist[str(dev)]), self.lens.iters, _lib.ptr(o["points_ideal"]),
            _lib.ptr(o["sigmas_ideal"]), _lib.ptr(o["lens_status"])), "spe_undistort_points")
        if stream is not None:
            # a converted copy was made on the current stream and is dropped here, while the kernel reads it
            # on `stream`
            for t, src in zip(ins, (points_px, sigmas, sigma_scale)):
                if t is not None and t is not src:
                    t.record_stream(stream)
        return o

    def _prologue(self, points_px, probs, sigmas, sigma_scale, undistorted, stream):
        """Every solve_batch's start: the device constants, the world check and, with a lens, the undistortion.
        -> K, the landmarks, the (points, sigmas) to solve on and what `out` gains."""
        B, Q, C = probs.shape
        Kd, Wd = self._consts(probs.device)
        self._check_world(C)
        ideal = {}
        if self.lens is not None and not undistorted and B > 0:
            o = self.undistort(points_px, sigmas, sigma_scale, stream)
            points_px, sigmas, ideal = o["points_ideal"], o["sigmas_ideal"], {k: v for k, v in o.items() if v is not None}
        return Kd, Wd, points_px, sigmas, ideal

    @staticmethod
    def _pose_tensors(B, dev):
        """The seven outputs every solver kernel fills."""
        return dict(quat=torch.empty(B, 4, device=dev), tvec=torch.empty(B, 3, dtype=torch.float64, device=dev),
                    rvec=torch.empty(B, 3, dtype=torch.float64, device=dev),
                    status=torch.empty(B, dtype=torch.int32, device=dev),
                    n_corr=torch.empty(B, dtype=torch.int32, device=dev),
                    corr_label=torch.empty(B, 16, dtype=torch.int32, device=dev),
                    inlier_mask=torch.empty(B, dtype=torch.int32, device=dev))

    def _consts(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.as_tensor(self.K, dtype=torch.float64, device=device).contiguous(),
                              torch.as_tensor(self.W_Pt, dtype=torch.float64, device=device).contiguous())
        return self._dev[key]

    def solve_batch(self, points_px, probs, sigmas=None, stream=None, out=None, repro_per_image=None,
                    sigma_scale=None, undistorted=False):
        """points_px [B,Q,2], probs [B,Q,C] (+ sigmas [B,Q,2]) device fp32 -> dict of device
        tensors quat [B,4] f32, tvec [B,3] f64, rvec, status, n_corr, corr_label [B,16],
        inlier_mask [B].  repro_per_image: device fp32 [B] thresholds replacing
        reprojectionError image by image (EPnPCeresSolver).

        With a lens the points and sigmas first go through undistort() and the solver runs on its
        buffers; the result also carries points_ideal, sigmas_ideal (with sigmas) and lens_status.
        sigma_scale [B,2]: the pixels per sigma unit (sigma_scale_of(clip_bbox) for a model's
        crop-normalised sigmas; None: they are pixels).  undistorted: the points are ideal already."""
        B, Q, C = probs.shape
        Kd, Wd, points_px, sigmas, ideal = self._prologue(points_px, probs, sigmas, sigma_scale, undistorted, stream)
        if out is None:
            out = self._pose_tensors(B, probs.device)
        _lib.check(_lib.lib().spe_pnp_batch(
            _lib.stream_ptr(stream), _lib.ptr(points_px.contiguous()), _lib.ptr(probs.contiguous()),
            _lib.ptr(sigmas.contiguous() if sigmas is not None else None), B, Q, C, _lib.ptr(Kd), _lib.ptr(Wd),
            self.mode, self.reprojectionError, self.ransac_iters, self.confidence, _lib.ptr(out["quat"]),
            _lib.ptr(out["tvec"]), _lib.ptr(out["rvec"]), _lib.ptr(out["status"]), _lib.ptr(out["n_corr"]),
            _lib.ptr(out["corr_label"]), _lib.ptr(out["inlier_mask"]),
            _lib.ptr(repro_per_image.float().contiguous() if repro_per_image is not None else None)), "spe_pnp_batch")
        out.update(ideal)
        return out

    def self_assess(self, probs, sigmas, poses, score_th=0.5, sigma_th=5.0, min_inliers=4, stream=None):
        """Self-assessment filter over a solve_batch result (BASELINE config 4; definition and
        its unpinned status: include/spe.h spe_self_assess, after the commented gate of
        UNC/utils/speed_eval_ceres.py:110-114).  Returns device tensors mean_sigma [B] f32,
        n_confident [B] i32, reliable [B] bool."""
        B, Q, C = probs.shape
        dev = probs.device
        out = dict(mean_sigma=torch.empty(B, device=dev), n_confident=torch.empty(B, dtype=torch.int32, device=dev),
                   reliable=torch.empty(B, dtype=torch.uint8, device=dev))
        _lib.check(_lib.lib().spe_self_assess(
            _lib.stream_ptr(stream), _lib.ptr(probs.contiguous()), _lib.ptr(sigmas.contiguous()),
            _lib.ptr(poses["status"]), _lib.ptr(poses["corr_label"]), _lib.ptr(poses["inlier_mask"]), B, Q, C,
            float(score_th), float(sigma_th), int(min_inliers), _lib.ptr(out["mean_sigma"]),
            _lib.ptr(out["n_confident"]), _lib.ptr(out["reliable"])), "spe_self_assess")
        out["reliable"] = out["reliable"].bool()
        return out

    def pose_covariance(self, probs, sigmas, poses, clip_bbox=None, sigma_floor=1e-3, stream=None, sigma_gain=1.0):
        """First-order covariance of a solve_batch result's poses from the keypoint sigmas (definition:
        include/spe.h spe_pose_covariance).  `poses` is solve_batch's dict of any solver class (status,
        corr_label, inlier_mask, rvec, tvec).  clip_bbox [B,4] (x1, y1, x2, y2): the sigmas are
        crop-normalised and scale to pixels by the crop's width and height, the factor PostProcess
        applies to the points; None: they are in pixels.  Returns device tensors pose_cov [B,6,6] f64
        (state order: rotation rad, translation m), sigma_rot [B] f32, sigma_t [B,3] f64, pred_score [B]
        f32 and cov_status [B] i32 (0 ok, 1 no pose, 2 fewer than 3 inliers, 3 bad sigma, 4 singular;
        the numeric outputs of a non-zero status are 0).  Poses solved through a lens carry
        sigmas_ideal, the sigmas in the image the pose was solved in: those are used.  sigma_gain: a
        calibration factor on every sigma (spe.calibration measures it), multiplied into the scale -- without
        a clip_bbox a [B,2] scale of the gain is made; at 1.0 nothing changes, bit for bit."""
        B, Q, C = probs.shape
        sigma_gain = float(sigma_gain)
        if not 0 < sigma_gain < float("inf"):
            raise ValueError(f"sigma_gain must be positive and finite, got {sigma_gain}")
        sigmas = poses.get("sigmas_ideal", sigmas)
        dev = probs.device
        Kd, Wd = self._consts(dev)
        if C - 1 > Wd.shape[0]:
            raise ValueError(f"pose_covariance: {C} classes need {C - 1} landmarks, the solver holds {Wd.shape[0]}")
        out = dict(pose_cov=torch.empty(B, 6, 6, dtype=torch.float64, device=dev), sigma_rot=torch.empty(B, device=dev),
                   sigma_t=torch.empty(B, 3, dtype=torch.float64, device=dev), pred_score=torch.empty(B, device=dev),
                   cov_status=torch.empty(B, dtype=torch.int32, device=dev))
        if B == 0:
            return out
        scale = None
        if clip_bbox is not None:
            # made on the stream the kernel reads it on
            scale = sigma_scale_of(clip_bbox, dev, stream)
        if sigma_gain != 1.0:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
                scale = scale * sigma_gain if scale is not None else torch.full((B, 2), sigma_gain, device=dev)
        _lib.check(_lib.lib().spe_pose_covariance(
            _lib.stream_ptr(stream), _lib.ptr(probs.contiguous()), _lib.ptr(sigmas.contiguous()), _lib.ptr(scale),
            _lib.ptr(poses["status"]), _lib.ptr(poses["corr_label"]), _lib.ptr(poses["inlier_mask"]),
            _lib.ptr(poses["rvec"]), _lib.ptr(poses["tvec"]), B, Q, C, _lib.ptr(Kd), _lib.ptr(Wd), float(sigma_floor),
            _lib.ptr(out["pose_cov"]), _lib.ptr(out["sigma_rot"]), _lib.ptr(out["sigma_t"]), _lib.ptr(out["pred_score"]),
            _lib.ptr(out["cov_status"])), "spe_pose_covariance")
        return out

    def find_index(self, logits):
        return logits.argmax(1), logits.max(1)

    def __call__(self, points, logits, sigmas=None, device=None, undistorted=False):
        """One image, numpy in / numpy out (REV/utils/speed_eval.py:164-242)."""
        points = np.asarray(points, dtype=np.float32)
        logits = np.asarray(logits, dtype=np.float32)
        assert points.shape[0] == logits.shape[0], "[Solver]: num_queries!"
        dev = device or torch.device("cuda")
        p = torch.from_numpy(points[None].copy()).to(dev)
        l = torch.from_numpy(logits[None].copy()).to(dev)
        s = torch.from_numpy(np.asarray(sigmas, np.float32)[None].copy()).to(dev) if sigmas is not None else None
        o = self.solve_batch(p, l, s, undistorted=True) if undistorted else self.solve_batch(p, l, s)
        st = int(o["status"][0].item())
        if st == _lib.SPE_PNP_NO_FG:
            raise IndexError("no foreground keypoint")
        if st in (_lib.SPE_PNP_CV_ERROR, _lib.SPE_PNP_UNPINNED):
            raise SolverError(f"solver status {st}")
        return o["quat"][0].double().cpu().numpy(), o["tvec"][0].cpu().numpy()


class SimplePoseSolver(PoseSolver):
    """cv2.solvePnPRansac(P3P, reprojectionError=args.repro) + solvePnPGeneric(ITERATIVE)
    (REV/utils/speed_eval.py:143-242)."""

    def __init__(self, args=None, lens=None, world=None):
        super().__init__(_lib.SPE_PNP_RANSAC_P3P_LM, getattr(args, "repro", 20) if args is not None else 20,
                         lens=lens, world=world)


class SimplePoseSolverSigma(PoseSolver):
    """EPnP-RANSAC (reprojection 25) + sigma-weighted Huber LM (UNC/utils/speed_eval.py:322-420)."""

    def __init__(self, args=None, lens=None, world=None):
        super().__init__(_lib.SPE_PNP_EPNP_RANSAC_SIGMA, 25.0, lens=lens, world=world)


class EPnPSolver(PoseSolver):
    """solvePnPGeneric(EPNP) on all selected points (UNC/utils/speed_eval_ceres.py:153-169, epnp_init);
    BASELINE config 2 ("EPnP only, no RANSAC").  inlier_mask: epnp_init's set, reprojection error
    < reprojectionError."""

    def __init__(self, args=None, refine=False, lens=None, world=None):
        super().__init__(_lib.SPE_PNP_EPNP_LM if refine else _lib.SPE_PNP_EPNP, 20.0, lens=lens, world=world)


class EPnPCeresSolver(PoseSolver):
    """UNC EPnPCeresSolver (UNC/utils/speed_eval_ceres.py:43-243): EPnP on every selected point,
    inliers = reprojection error < the threshold of the image's box area (get_repro_th), the
    sigma-weighted Huber(0.001) LM on the inliers, and the EPnP pose kept when the refined error
    sum over all points is larger.  A batch carries one threshold per image."""

    def __init__(self, input_size=256, lens=None, world=None):
        super().__init__(_lib.SPE_PNP_EPNP_CERES, 20.0, lens=lens, world=world)
        self.input_size = input_size

    def repro_th(self, area):
        """The threshold of one box area (UNC/utils/speed_eval_ceres.py:53-58: int() truncation, then
        [1.5, 20]) without touching the solver's state."""
        repro = int(area / self.input_size * 10)
        return float(min(max(repro, 1.5), 20))

    def get_repro_th(self, area):
        """UNC/utils/speed_eval_ceres.py:53-58: sets reprojectionError for the next __call__, as the
        reference does (its per-image call path)."""
        self.reprojectionError = self.repro_th(area)
        return self.reprojectionError

    def _thresholds(self, repro_per_image, area, dev, stream):
        """`repro_per_image`, or `area` (B box areas, repro_th each) -> the device fp32 [B] thresholds, kept for
        `stream` (the kernel may still read them there after solve_batch returns); None with neither."""
        if repro_per_image is None:
            if area is None:
                return None
            repro_per_image = torch.tensor([self.repro_th(float(a)) for a in area], dtype=torch.float32, device=dev)
        repro_per_image = repro_per_image.float().contiguous()
        if stream is not None:
            repro_per_image.record_stream(stream)
        return repro_per_image

    def solve_batch(self, points_px, probs, sigmas=None, stream=None, out=None, repro_per_image=None, area=None,
                    sigma_scale=None, undistorted=False):
        """As PoseSolver.solve_batch with one threshold per image: `area` (B box areas) or
        `repro_per_image` (device fp32 [B]) is required -- the reference has no batch-wide
        threshold for this solver (get_repro_th runs per image, :90)."""
        repro_per_image = self._thresholds(repro_per_image, area, probs.device, stream)
        if repro_per_image is None:
            raise ValueError("EPnPCeresSolver.solve_batch needs the per-image box areas (area=) or thresholds "
                             "(repro_per_image=): the reference derives every image's threshold from its area")
        o = super().solve_batch(points_px, probs, sigmas, stream=stream, out=out, repro_per_image=repro_per_image,
                                sigma_scale=sigma_scale, undistorted=undistorted)
        o["repro_per_image"] = repro_per_image
        return o

    def __call__(self, points, logits, area, sigma, device=None):
        """One image, the reference's signature (:70): numpy in / numpy out."""
        self.get_repro_th(area)
        return PoseSolver.__call__(self, points, logits, sigma, device=device)


class ExhaustivePoseSolver(PoseSolver):
    """UNC PoseSolver(pnp_method="exhausive") behind SimplePoseSolver.__call__
    (UNC/utils/speed_eval_ceres.py:326-399, :465-522): EPnP on every four-point subset of the selected
    correspondences, the `topk` smallest four-point errors, and per kept hypothesis the inliers over
    all points (threshold + 5 whenever fewer than 4), the sigma-weighted Huber(0.001) LM on them and
    revert-if-worse; the candidate with the smallest error sum wins.  Draws no samples: the result is a
    function of the correspondences alone.  What is unpinned: include/spe.h, SPE_PNP_EXHAUSTIVE."""

    def __init__(self, topk=10, input_size=256, repro=20.0, lens=None, world=None):
        topk = int(topk)
        if not 1 <= topk <= 64:
            raise ValueError(f"topk must be in [1, 64], got {topk}")
        super().__init__(_lib.SPE_PNP_EXHAUSTIVE, repro, lens=lens, world=world)
        self.topk = topk
        self.input_size = input_size

    repro_th = EPnPCeresSolver.repro_th
    get_repro_th = EPnPCeresSolver.get_repro_th
    _thresholds = EPnPCeresSolver._thresholds

    def solve_batch(self, points_px, probs, sigmas=None, stream=None, out=None, repro_per_image=None, area=None,
                    sigma_scale=None, undistorted=False):
        """As PoseSolver.solve_batch plus cand_index [B] i32 (the winner's subset index, -1 without a
        pose) and repro_final [B] f32 (the threshold after growth).  `area` (B box areas, get_repro_th
        each) or `repro_per_image` (device fp32 [B]) gives one threshold per image; with neither the
        batch-wide reprojectionError is used."""
        B, Q, C = probs.shape
        dev = probs.device
        Kd, Wd, points_px, sigmas, ideal = self._prologue(points_px, probs, sigmas, sigma_scale, undistorted, stream)
        repro_per_image = self._thresholds(repro_per_image, area, dev, stream)
        if out is None:
            out = self._pose_tensors(B, dev)
        for k, dt in (("cand_index", torch.int32), ("repro_final", torch.float32)):
            if k not in out:
                out[k] = torch.empty(B, dtype=dt, device=dev)
        _lib.check(_lib.lib().spe_pnp_exhaustive(
            _lib.stream_ptr(stream), _lib.ptr(points_px.contiguous()), _lib.ptr(probs.contiguous()),
            _lib.ptr(sigmas.contiguous() if sigmas is not None else None), B, Q, C, _lib.ptr(Kd), _lib.ptr(Wd),
            self.reprojectionError, self.topk, _lib.ptr(out["quat"]), _lib.ptr(out["tvec"]), _lib.ptr(out["rvec"]),
            _lib.ptr(out["status"]), _lib.ptr(out["n_corr"]), _lib.ptr(out["corr_label"]),
            _lib.ptr(out["inlier_mask"]), _lib.ptr(repro_per_image), _lib.ptr(out["cand_index"]),
            _lib.ptr(out["repro_final"])), "spe_pnp_exhaustive")
        out.update(ideal)
        if repro_per_image is not None:
            out["repro_per_image"] = repro_per_image
        return out

    def __call__(self, points, logits, area, sigma=None, device=None):
        """One image, the reference's signature (:473) plus the optional sigmas: numpy in / numpy out."""
        self.get_repro_th(area)
        return PoseSolver.__call__(self, points, logits, sigma, device=device)


class Multi_Mean_PoseSolver(PoseSolver):
    """Multi-checkpoint ensemble (REV/utils/speed_eval.py:42-140): the M models' keypoints are
    fused per label (mean after a 3-sigma filter, first-seen label order) on the device
    (spe_ensemble_fuse) and solved like SimplePoseSolver (P3P-RANSAC + LM).  With a lens every model's
    points are undistorted before the fusion, in one launch over [M * B, Q]."""

    def __init__(self, args=None, lens=None, world=None):
        super().__init__(_lib.SPE_PNP_RANSAC_P3P_LM, getattr(args, "repro", 25) if args is not None else 25,
                         lens=lens, world=world)

    def fuse_batch(self, multi_points_px, multi_probs, stream=None):
        """lists of M device tensors [B,Q,2] / [B,Q,C] -> fused points [B,C-1,2], probs [B,C-1,C]."""
        pts = torch.stack(list(multi_points_px)).float().contiguous()
        prb = torch.stack(list(multi_probs)).float().contiguous()
        M, B, Q, C = prb.shape
        if self.lens is not None and B > 0:
            if stream is not None:
                pts.record_stream(stream)      # the stacked copy is read on `stream` and dropped here
            pts = self.undistort(pts.view(M * B, Q, 2), stream=stream)["points_ideal"].view(M, B, Q, 2)
        fp = torch.empty(B, C - 1, 2, device=prb.device)
        fr = torch.empty(B, C - 1, C, device=prb.device)
        _lib.check(_lib.lib().spe_ensemble_fuse(_lib.stream_ptr(stream), _lib.ptr(pts), _lib.ptr(prb), M, B, Q, C,
                                                _lib.ptr(fp), _lib.ptr(fr)), "spe_ensemble_fuse")
        return fp, fr

    def solve_batch_multi(self, multi_points_px, multi_probs, stream=None):
        fp, fr = self.fuse_batch(multi_points_px, multi_probs, stream=stream)
        return self.solve_batch(fp, fr, stream=stream, undistorted=True)

    def __call__(self, multi_points, multi_logits, device=None):
        """One image, numpy lists in / numpy out, the reference's call (gen_submission)."""
        assert isinstance(multi_points, list) and isinstance(multi_logits, list)
        assert len(multi_points) == len(multi_logits)
        dev = device or torch.device("cuda")
        mp = [torch.from_numpy(np.asarray(p, np.float32)[None].copy()).to(dev) for p in multi_points]
        ml = [torch.from_numpy(np.asarray(l, np.float32)[None].copy()).to(dev) for l in multi_logits]
        fp, fr = self.fuse_batch(mp, ml)
        return PoseSolver.__call__(self, fp[0].cpu().numpy(), fr[0].cpu().numpy(), device=dev, undistorted=True)


class SigmaEnsemblePoseSolver:
    """Multi-checkpoint ensemble of sigma models: per label one measurement per model, fused by a gated
    inverse-variance mean into a point with a sigma (spe_ensemble_fuse_sigma; the rule, which has no
    reference counterpart, is defined in include/spe.h), then solved by `backend` -- any solver object of
    this module, SimplePoseSolverSigma by default -- with the fused sigma.  The fused arrays have
    solve_batch's layout, so the backend's self_assess and pose_covariance take them as they take one
    model's.  With a lens every model's points and sigmas are undistorted before the fusion, in one launch
    over [M * B, Q], and the fused arrays are ideal.  The lens is the backend's.  lens=: NOTE that it is
    installed ON THE BACKEND OBJECT passed in (set_lens: its K is replaced and it undistorts from then on,
    also when called directly); a backend that already holds another lens is refused.  world=: a landmark
    table, installed on the backend object too (set_world)."""

    def __init__(self, backend=None, gate=3.0, sigma_floor=1e-3, lens=None, world=None):
        self.backend = backend if backend is not None else SimplePoseSolverSigma()
        if not hasattr(self.backend, "solve_batch"):
            raise ValueError("SigmaEnsemblePoseSolver: the backend must be a solver object (solve_batch)")
        if world is not None:
            self.backend.set_world(world)      # like lens=: installed on the backend object
        if lens is not None:
            if getattr(self.backend, "lens", None) not in (None, lens):
                raise ValueError("SigmaEnsemblePoseSolver: the backend already holds a different lens")
            if self.backend.lens is None:
                self.backend.set_lens(lens)
        self.gate = float(gate)
        self.sigma_floor = float(sigma_floor)
        if not self.gate > 0:
            raise ValueError(f"gate must be positive, got {gate}")
        if not 0 < self.sigma_floor < float("inf"):
            raise ValueError(f"sigma_floor must be positive and finite, got {sigma_floor}")

    @property
    def mode(self):
        return self.backend.mode

    @property
    def lens(self):
        return getattr(self.backend, "lens", None)

    def fuse_batch(self, multi_points_px, multi_probs, multi_sigmas, clip_bbox=None, stream=None):
        """lists of M device tensors [B,Q,2] / [B,Q,C] / [B,Q,2] -> dict of device tensors points
        [B,C-1,2], probs [B,C-1,C], sigmas [B,C-1,2] f32, n_pooled, n_kept [B,C-1] i32.  clip_bbox [B,4]
        (x1, y1, x2, y2): the sigmas are crop-normalised and weigh in pixels, by the crop's width and
        height; the fused sigma is crop-normalised again.  None: they are in the points' unit.  With a
        lens also lens_status [M,B,Q] u8 (PoseSolver.undistort)."""
        if multi_sigmas is None:
            raise ValueError("SigmaEnsemblePoseSolver needs every model's sigmas (multi_sigmas)")
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            pts = torch.stack(list(multi_points_px)).float().contiguous()
            prb = torch.stack(list(multi_probs)).float().contiguous()
            sig = torch.stack(list(multi_sigmas)).float().contiguous()
            M, B, Q, C = prb.shape
            dev = prb.device
            scale = sigma_scale_of(clip_bbox, dev, stream) if clip_bbox is not None else None
            lens_scale = scale.repeat(M, 1) if scale is not None and self.lens is not None else None
        if pts.shape != (M, B, Q, 2) or sig.shape != (M, B, Q, 2):
            raise ValueError(f"points {tuple(pts.shape)} / sigmas {tuple(sig.shape)} do not match probs {tuple(prb.shape)}")
        lens_status = None
        if self.lens is not None and B > 0:
            u = self.backend.undistort(pts.view(M * B, Q, 2), sig.view(M * B, Q, 2), lens_scale, stream)
            if stream is not None:
                for t in (pts, sig) + ((lens_scale,) if lens_scale is not None else ()):
                    t.record_stream(stream)
            pts, sig = u["points_ideal"].view(M, B, Q, 2), u["sigmas_ideal"].view(M, B, Q, 2)
            lens_status = u["lens_status"].view(M, B, Q)
        out = dict(points=torch.empty(B, C - 1, 2, device=dev), probs=torch.empty(B, C - 1, C, device=dev),
                   sigmas=torch.empty(B, C - 1, 2, device=dev),
                   n_pooled=torch.empty(B, C - 1, dtype=torch.int32, device=dev),
                   n_kept=torch.empty(B, C - 1, dtype=torch.int32, device=dev))
        if lens_status is not None:
            out["lens_status"] = lens_status
        if B == 0:
            return out
        _lib.check(_lib.lib().spe_ensemble_fuse_sigma(
            _lib.stream_ptr(stream), _lib.ptr(pts), _lib.ptr(prb), _lib.ptr(sig), _lib.ptr(scale), M, B, Q, C,
            self.sigma_floor, self.gate, _lib.ptr(out["points"]), _lib.ptr(out["probs"]), _lib.ptr(out["sigmas"]),
            _lib.ptr(out["n_pooled"]), _lib.ptr(out["n_kept"])), "spe_ensemble_fuse_sigma")
        if stream is not None:
            # the kernel may still read its inputs on `stream` after this returns
            for t in (pts, prb, sig) + ((scale,) if scale is not None else ()):
                t.record_stream(stream)
        return out

    def solve_batch_multi(self, multi_points_px, multi_probs, multi_sigmas=None, clip_bbox=None, area=None,
                          repro_per_image=None, stream=None):
        """Fuses, then the backend's solve_batch on the fused arrays with the fused sigma.  area /
        repro_per_image go to the solvers that take them (EPnPCeresSolver, ExhaustivePoseSolver).  Returns
        the backend's pose dict plus "fused", fuse_batch's dict."""
        fused = self.fuse_batch(multi_points_px, multi_probs, multi_sigmas, clip_bbox=clip_bbox, stream=stream)
        kw = {}
        if self.lens is not None:
            kw["undistorted"] = True           # fuse_batch undistorted every model's points and sigmas
        if area is not None:
            kw["area"] = area
        if repro_per_image is not None:
            kw["repro_per_image"] = repro_per_image
        poses = self.backend.solve_batch(fused["points"], fused["probs"], fused["sigmas"], stream=stream, **kw)
        poses["fused"] = fused
        return poses

    def set_world(self, world):
        self.backend.set_world(world)

    @property
    def W_Pt(self):
        return self.backend.W_Pt

    def self_assess(self, probs, sigmas, poses, **kw):
        return self.backend.self_assess(probs, sigmas, poses, **kw)

    def pose_covariance(self, probs, sigmas, poses, **kw):
        return self.backend.pose_covariance(probs, sigmas, poses, **kw)


def build_solver(args=None):
    """REV/utils/speed_eval.py:21-22 (SimplePoseSolver); `args.solver` selects the variant.
    "ensemble_sigma" wraps the solver `args.backend` names (epnp_ransac_sigma by default) in a
    SigmaEnsemblePoseSolver with `args.gate` / `args.sigma_floor`.  `args.dist` (4 or 5 OpenCV distortion
    coefficients), when present, gives the solver a lens (LensModel.from_args); `args.world` (a path to a
    world_points.json-style file, an [L,3] array or a LandmarkModel) its landmark table (load_world)."""
    name = getattr(args, "solver", "ransac_p3p_lm") if args is not None else "ransac_p3p_lm"
    lens = LensModel.from_args(args) if getattr(args, "dist", None) is not None else None
    world = getattr(args, "world", None)
    if name == "ensemble_sigma":
        import argparse
        backend = getattr(args, "backend", "epnp_ransac_sigma")
        if backend == "ensemble_sigma":
            raise ValueError("ensemble_sigma cannot be its own backend")
        inner = argparse.Namespace(**{**vars(args), "solver": backend})
        return SigmaEnsemblePoseSolver(build_solver(inner), getattr(args, "gate", 3.0),
                                       getattr(args, "sigma_floor", 1e-3))
    if name == "ransac_p3p_lm":
        return SimplePoseSolver(args, lens=lens, world=world)
    if name == "epnp_ransac_sigma":
        return SimplePoseSolverSigma(args, lens=lens, world=world)
    if name in ("epnp", "epnp_lm"):
        return EPnPSolver(args, refine=name == "epnp_lm", lens=lens, world=world)
    if name == "epnp_ceres":
        return EPnPCeresSolver(getattr(args, "input_size", 256) if args is not None else 256, lens=lens, world=world)
    if name == "exhaustive":
        return ExhaustivePoseSolver(getattr(args, "topk", 10), getattr(args, "input_size", 256),
                                    getattr(args, "repro", 20.0), lens=lens, world=world)
    raise ValueError(f"unknown solver {name}")
