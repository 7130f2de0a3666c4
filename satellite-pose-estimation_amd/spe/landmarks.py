"""Reconstruction of the 3-D landmark table from posed 2-D keypoint observations (definition: include/spe.h
spe_landmarks_solve; the paper's multi-view triangulation, whose code the reference does not ship -- it ships
the finished table, spe/data/world_points.json).

    rec = LandmarkReconstruction(num_landmarks=11)             # lens=solver.lens for a distorting camera
    for batch in posed_set:                                    # ground-truth poses q_gt [B,4], t_gt [B,3]
        rec.update(out["points_px"], out["probs"], out["sigmas"], q_gt, t_gt, sigma_scale=sigma_scale_of(clip))
        # or, from annotated points [B,L,2]:  rec.update_annotations(landmarks, q_gt, t_gt)
    model = rec.solve()                                        # the one host synchronisation
    model.save("my_target.json")                               # world_points.json's layout
    solver = build_solver(Namespace(solver="epnp", world="my_target.json"))      # or SimplePoseSolver(world=model)

update() never synchronises with the host: the observations stay on the device in buffers that grow by
doubling, and the selection kernel (spe_landmark_observations) writes each batch at its row.  solve() runs
the fixed launch sequence of spe_landmarks_solve and downloads the result.  evaluate(..., landmarks=rec) and
evaluate_rtdetr(..., landmarks=rec) call update() per batch.
"""
from __future__ import annotations

import json
import math

import numpy as np
import torch

from . import _lib
from .config import Camera

MAX_LANDMARKS = 16


class LandmarkModel:
    """The result of LandmarkReconstruction.solve, numpy on the host: points [L,3] m, cov [L,3,3] (H^-1 at the
    point, unit-sigma), chi2 [L] (the robust cost), n_used [L], rms_px [L], status [L] (0 ok, 1 fewer than 2
    usable views, 2 degenerate, 3 not finite; the numbers of a non-zero status are 0) and obs_flags [N,L] u8
    (bit 0 used, bit 1 beyond the Huber threshold)."""

    def __init__(self, points, cov, chi2, n_used, rms_px, status, obs_flags, source="spe.landmarks"):
        self.points = np.asarray(points, np.float64)
        self.cov = np.asarray(cov, np.float64)
        self.chi2 = np.asarray(chi2, np.float64)
        self.n_used = np.asarray(n_used, np.int32)
        self.rms_px = np.asarray(rms_px, np.float64)
        self.status = np.asarray(status, np.int32)
        self.obs_flags = np.asarray(obs_flags, np.uint8)
        self.source = source

    def birge(self):
        """Per landmark max(1, chi2 / (2 n - 3)): the Birge ratio of 2 n residuals and 3 parameters, never
        below 1 (1 for a landmark without a solution)."""
        dof = 2 * self.n_used.astype(np.float64) - 3
        return np.where((self.status == 0) & (dof > 0), np.maximum(1.0, self.chi2 / np.maximum(dof, 1.0)), 1.0)

    @property
    def cov_scaled(self):
        """cov times the Birge ratio: the covariance when the sigmas were too small."""
        return self.cov * self.birge()[:, None, None]

    def save(self, path, source=None):
        """Writes world_points.json's layout: {"source", "points"}."""
        with open(path, "w") as f:
            json.dump({"source": source if source is not None else self.source, "points": self.points.tolist()}, f,
                      indent=1)

    def compare(self, other_points):
        """Per-landmark distance (m) to another table ([L,3], or a LandmarkModel)."""
        other = np.asarray(getattr(other_points, "points", other_points), np.float64)
        if other.shape != self.points.shape:
            raise ValueError(f"compare: {other.shape} against {self.points.shape}")
        return np.linalg.norm(self.points - other, axis=1)


def _positive(v, name):
    v = float(v)
    if not (v > 0 and math.isfinite(v)):
        raise ValueError(f"{name} must be positive and finite, got {v}")
    return v


class LandmarkReconstruction:
    """Accumulates posed keypoint observations on the device and solves for the landmarks (module docstring).
    K: the camera matrix (None: Camera.K, or the lens's).  lens (a spe.config.LensModel): the points and their
    sigmas first pass through spe_undistort_points, as in front of the solvers.  huber: the robust threshold
    in sigma units (<= 0: off); sigma_floor, sigma_gain: the covariance's sigma rule; z_min: the smallest camera
    depth (m) a view is used at.  Everything runs on the current stream."""

    def __init__(self, num_landmarks=11, K=None, lens=None, huber=3.0, sigma_floor=1e-3, sigma_gain=1.0, z_min=0.1):
        self.L = int(num_landmarks)
        if not 1 <= self.L <= MAX_LANDMARKS:
            raise ValueError(f"num_landmarks must be in [1, {MAX_LANDMARKS}], got {num_landmarks}")
        self.lens = lens
        self.K = np.array(K if K is not None else (lens.K if lens is not None else Camera.K), np.float64).reshape(3, 3)
        self.huber = float(huber)
        self.sigma_floor = _positive(sigma_floor, "sigma_floor")
        self.sigma_gain = _positive(sigma_gain, "sigma_gain")
        self.z_min = float(z_min)
        self.n = 0
        self._buf = None
        self._dev = {}

    def _consts(self, dev):
        key = str(dev)
        if key not in self._dev:
            dist = torch.tensor(self.lens.dist.tolist(), dtype=torch.float64, device=dev) if self.lens is not None else None
            self._dev[key] = (torch.as_tensor(self.K, dtype=torch.float64, device=dev).contiguous(), dist)
        return self._dev[key]

    def _reserve(self, B, dev):
        """Room for B more views: the buffers double (no host synchronisation)."""
        cap = 0 if self._buf is None else self._buf["q"].shape[0]
        if self.n + B <= cap:
            return self._buf
        cap = max(2 * cap, self.n + B, 256)
        new = dict(px=torch.zeros(cap, self.L, 2, dtype=torch.float64, device=dev),
                   sigma=torch.ones(cap, self.L, 2, dtype=torch.float64, device=dev),
                   valid=torch.zeros(cap, self.L, dtype=torch.uint8, device=dev),
                   q=torch.zeros(cap, 4, dtype=torch.float64, device=dev),
                   t=torch.zeros(cap, 3, dtype=torch.float64, device=dev))
        if self._buf is not None:
            for k, v in self._buf.items():
                new[k][:self.n] = v[:self.n]
        self._buf = new
        return new

    def _undistort(self, points, sigmas, sigma_scale):
        """float32 [B,Q,2] points (+ sigmas) through the lens -> ideal points, sigmas in the same unit"""
        B, Q = points.shape[:2]
        Kd, dist = self._consts(points.device)
        po = torch.empty_like(points)
        so = torch.empty_like(sigmas) if sigmas is not None else None
        _lib.check(_lib.lib().spe_undistort_points(
            _lib.stream_ptr(), _lib.ptr(points), _lib.ptr(sigmas), _lib.ptr(sigma_scale), B, Q, _lib.ptr(Kd),
            _lib.ptr(dist), self.lens.iters, _lib.ptr(po), _lib.ptr(so), None), "spe_undistort_points")
        return po, so

    def _poses(self, buf, q_gt, t_gt, B, dev):
        q = torch.as_tensor(q_gt).to(device=dev, dtype=torch.float64)
        t = torch.as_tensor(t_gt).to(device=dev, dtype=torch.float64)
        if q.shape != (B, 4) or t.shape != (B, 3):
            raise ValueError(f"q_gt {tuple(q.shape)} / t_gt {tuple(t.shape)} do not match a batch of {B}")
        buf["q"][self.n:self.n + B] = q
        buf["t"][self.n:self.n + B] = t

    def update(self, points_px, probs, sigmas, q_gt, t_gt, sigma_scale=None):
        """One batch of model output: points_px [B,Q,2], probs [B,Q,C] with C - 1 = num_landmarks, sigmas
        [B,Q,2] or None (1 px), sigma_scale [B,2] the pixels per sigma unit (sigma_scale_of(clip_bbox) for a
        model's crop-normalised sigmas; None: they are pixels), and the views' ground-truth poses.  One
        selection launch (two with a lens); no host synchronisation."""
        B, Q, C = probs.shape
        if C - 1 != self.L:
            raise ValueError(f"update: {C} classes give {C - 1} landmarks, this reconstruction holds {self.L}")
        if B == 0:
            return
        dev = probs.device
        buf = self._reserve(B, dev)
        pts = points_px.float().contiguous()
        sig = sigmas.float().contiguous() if sigmas is not None else None
        scale = sigma_scale.float().contiguous() if sigma_scale is not None and sig is not None else None
        if self.lens is not None:
            pts, sig = self._undistort(pts, sig, scale)
        self._poses(buf, q_gt, t_gt, B, dev)
        _lib.check(_lib.lib().spe_landmark_observations(
            _lib.stream_ptr(), _lib.ptr(pts), _lib.ptr(probs.float().contiguous()), _lib.ptr(sig), _lib.ptr(scale),
            B, Q, C, self.n, _lib.ptr(buf["px"]), _lib.ptr(buf["sigma"]), _lib.ptr(buf["valid"])),
            "spe_landmark_observations")
        self.n += B

    def update_annotations(self, landmarks, q_gt, t_gt, valid=None):
        """One batch of annotated points: landmarks [B,L,2] pixels (sigma 1 px), valid [B,L] or None (all)."""
        lm = torch.as_tensor(landmarks)
        if lm.dim() != 3 or lm.shape[1:] != (self.L, 2):
            raise ValueError(f"update_annotations: landmarks {tuple(lm.shape)}, expected [B, {self.L}, 2]")
        B = lm.shape[0]
        if B == 0:
            return
        dev = lm.device if lm.is_cuda else torch.device("cuda")
        buf = self._reserve(B, dev)
        lm = lm.to(dev)
        rows = slice(self.n, self.n + B)
        if self.lens is not None:
            # the lens kernel is fp32: the points round to fp32 pixels here
            po, so = self._undistort(lm.float().contiguous(), torch.ones(B, self.L, 2, device=dev), None)
            buf["px"][rows] = po.double()
            buf["sigma"][rows] = so.double()
        else:
            buf["px"][rows] = lm.double()
            buf["sigma"][rows] = 1.0
        buf["valid"][rows] = 1 if valid is None else (torch.as_tensor(valid).to(dev) != 0).to(torch.uint8)
        self._poses(buf, q_gt, t_gt, B, dev)
        self.n += B

    def observations(self):
        """The accumulated device tensors: obs_px, obs_sigma [N,L,2] f64, obs_valid [N,L] u8, q_gt, t_gt."""
        if self.n == 0:
            raise ValueError("LandmarkReconstruction: no observation was added")
        b = self._buf
        return dict(obs_px=b["px"][:self.n], obs_sigma=b["sigma"][:self.n], obs_valid=b["valid"][:self.n],
                    q_gt=b["q"][:self.n], t_gt=b["t"][:self.n])

    def solve_device(self, iterations=10, init=None):
        """spe_landmarks_solve on the accumulated observations -> dict of device tensors world, cov, chi2, n_used,
        rms_px, obs_flags, lm_status; no host synchronisation."""
        iterations = int(iterations)
        if not 0 <= iterations <= 64:
            raise ValueError(f"iterations must be in [0, 64], got {iterations}")
        o = self.observations()
        N, L = self.n, self.L
        dev = o["obs_px"].device
        Kd, _ = self._consts(dev)
        w0 = None
        if init is not None:
            w0 = torch.as_tensor(np.asarray(getattr(init, "points", init), np.float64), device=dev).contiguous()
            if w0.shape != (L, 3):
                raise ValueError(f"init {tuple(w0.shape)}, expected [{L}, 3]")
        nbytes = int(_lib.lib().spe_landmarks_scratch_bytes(N, L))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        out = dict(world=torch.empty(L, 3, **f64), cov=torch.empty(L, 3, 3, **f64), chi2=torch.empty(L, **f64),
                   n_used=torch.empty(L, dtype=torch.int32, device=dev), rms_px=torch.empty(L, **f64),
                   obs_flags=torch.empty(N, L, dtype=torch.uint8, device=dev),
                   lm_status=torch.empty(L, dtype=torch.int32, device=dev))
        _lib.check(_lib.lib().spe_landmarks_solve(
            _lib.stream_ptr(), _lib.ptr(o["obs_px"]), _lib.ptr(o["obs_sigma"]), _lib.ptr(o["obs_valid"]),
            _lib.ptr(o["q_gt"]), _lib.ptr(o["t_gt"]), N, L, _lib.ptr(Kd), _lib.ptr(w0), iterations, self.huber,
            self.sigma_floor, self.sigma_gain, self.z_min, _lib.ptr(scratch), nbytes, _lib.ptr(out["world"]),
            _lib.ptr(out["cov"]), _lib.ptr(out["chi2"]), _lib.ptr(out["n_used"]), _lib.ptr(out["rms_px"]),
            _lib.ptr(out["obs_flags"]), _lib.ptr(out["lm_status"])), "spe_landmarks_solve")
        return out

    def solve(self, iterations=10, init=None):
        """-> LandmarkModel (the one host synchronisation).  init: a start table [L,3] or a LandmarkModel instead
        of the linear stage."""
        o = {k: v.cpu().numpy() for k, v in self.solve_device(iterations, init).items()}
        return LandmarkModel(o["world"], o["cov"], o["chi2"], o["n_used"], o["rms_px"], o["lm_status"], o["obs_flags"],
                             source=f"spe.landmarks: {self.n} views, {int(iterations)} LM steps")
