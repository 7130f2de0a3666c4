"""Calibration of the predicted keypoint sigmas, pose covariances and predicted scores against ground
truth (definition: include/spe.h spe_calibration_records; the reference has no counterpart, its
self-assessment is commented out).

    cal = Calibration(solver=solver)                       # sigma_gain=1.0: the sigmas as predicted
    for batch in validation_set:
        poses = solver.solve_batch(points_px, probs, sigmas, ...)
        cov = solver.pose_covariance(probs, sigmas, poses, clip_bbox=clip)        # at its default gain
        s_t, s_q = device_speed_score(poses["quat"], poses["tvec"], q_gt, t_gt)
        cal.update(points_px, probs, sigmas, poses, cov, q_gt, t_gt, s_t, s_q, clip_bbox=clip)
    summary = cal.summarize()                              # the one host synchronisation
    g = summary["sigma_gain"]                              # the factor that makes the inliers' rms z equal 1

and Calibration(solver=solver, sigma_gain=g) over the same loop checks the calibrated sigmas and
covariances by the same code; sigma_gain=g on pose_covariance / PosePipeline / the evaluate loops then
applies the factor where the covariance is used.

The gain is applied by the kernel: update() takes the covariance at gain 1 (pose_covariance's default) and
the records read it as cov * gain^2, the sigmas as sigma * gain; the stored pred_score is pred_score * gain.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .config import Camera, world_points
from .solver import sigma_scale_of

# chi-square quantiles at 50 / 90 / 99 %.  How they were computed: bisection to the last bit on the closed-form
# distribution functions  F6(x) = 1 - exp(-x/2) (1 + x/2 + x^2/8)  and  F3(x) = erf(sqrt(x/2)) - sqrt(2x/pi) exp(-x/2)
# (tests/test_calibration.py evaluates both at these values).
CHI2_6 = (5.34812062744712, 10.64464067566842, 16.811893829770916)
CHI2_3 = (2.3659738843753377, 6.2513886311703235, 11.344866730144357)
STEPS = 20                      # the sparsification curve removes k / STEPS of the images, k = 0 .. STEPS - 1

RECORDS = ("delta", "nees", "z", "kp_flags", "calib_status")


def _check_gain(g):
    g = float(g)
    if not (g > 0 and math.isfinite(g)):
        raise ValueError(f"sigma_gain must be positive and finite, got {g}")
    return g


def calibration_records(points_px, probs, sigmas, poses, cov, q_gt, t_gt, clip_bbox=None, sigma_floor=1e-3,
                        sigma_gain=1.0, stream=None, solver=None):
    """spe_calibration_records, one launch: device tensors delta [B,6] f64 (rotation error rad, translation
    error m, in the covariance's perturbation convention), nees [B,3] f64 (full, rotation, translation),
    z [B,C-1,2] f64 (keypoint error over the effective sigma, per landmark and axis), kp_flags [B,C-1] u8
    (bit 0 valid, bit 1 taking-part inlier) and calib_status [B] i32 (0 ok, 1 ground truth unusable, 2 no
    pose, 3 no covariance, 4 singular).  poses: a solve_batch dict; cov: pose_covariance's dict at gain 1;
    clip_bbox as for pose_covariance.  Poses solved through a lens carry points_ideal / sigmas_ideal: those
    are used, the comparison is made in the image the pose was solved in.  solver: whose K and landmarks to
    use.  PASS THE SOLVER THAT SOLVED THE POSES whenever it is not a plain one: None means Camera.K and the 11
    SPEED landmarks, which is wrong for a solver with a lens (the lens's K) or with a K of its own; poses that
    carry points_ideal (a lens solved them) are refused without a solver."""
    B, Q, C = probs.shape
    dev = probs.device
    gain = _check_gain(sigma_gain)
    points_px = poses.get("points_ideal", points_px)
    sigmas = poses.get("sigmas_ideal", sigmas)
    backend = getattr(solver, "backend", solver)
    if backend is not None:
        Kd, Wd = backend._consts(dev)
    else:
        if "points_ideal" in poses:
            raise ValueError("calibration_records: these poses were solved through a lens; pass solver= (its K is the "
                             "lens's, not Camera.K)")
        Kd, Wd = _default_consts(dev)
    if C - 1 > Wd.shape[0]:
        raise ValueError(f"calibration_records: {C} classes need {C - 1} landmarks, {Wd.shape[0]} are given")
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        out = dict(delta=torch.empty(B, 6, dtype=torch.float64, device=dev),
                   nees=torch.empty(B, 3, dtype=torch.float64, device=dev),
                   z=torch.empty(B, C - 1, 2, dtype=torch.float64, device=dev),
                   kp_flags=torch.empty(B, C - 1, dtype=torch.uint8, device=dev),
                   calib_status=torch.empty(B, dtype=torch.int32, device=dev))
        if B == 0:
            return out
        scale = sigma_scale_of(clip_bbox, dev, st) if clip_bbox is not None else None
        ins = [points_px.float().contiguous(), probs.float().contiguous(), sigmas.float().contiguous()]
        gt = [q_gt.to(device=dev, dtype=torch.float64).contiguous(), t_gt.to(device=dev, dtype=torch.float64).contiguous()]
    _lib.check(_lib.lib().spe_calibration_records(
        _lib.stream_ptr(stream), _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), _lib.ptr(scale),
        float(sigma_floor), _lib.ptr(poses["status"]), _lib.ptr(poses["corr_label"]), _lib.ptr(poses["inlier_mask"]),
        _lib.ptr(poses["rvec"]), _lib.ptr(poses["tvec"]), _lib.ptr(gt[0]), _lib.ptr(gt[1]),
        _lib.ptr(cov["pose_cov"].contiguous()), _lib.ptr(cov["cov_status"]), B, Q, C, _lib.ptr(Kd), _lib.ptr(Wd), gain,
        *[_lib.ptr(out[k]) for k in RECORDS]), "spe_calibration_records")
    return out


_CONSTS = {}


def _default_consts(device):
    key = str(device)
    if key not in _CONSTS:
        _CONSTS[key] = (torch.as_tensor(Camera.K, dtype=torch.float64, device=device).contiguous(),
                        torch.as_tensor(world_points(), dtype=torch.float64, device=device).contiguous())
    return _CONSTS[key]


KP_SUMS = 8


def _keypoint_sums(z, mask):
    """-> 8 fp64 values (KP_SUMS): count, sum z (2), sum z^2, sum |z|, #(|z| <= 1, 2, 3) over the masked keypoints."""
    m = mask[..., None]
    zm = torch.where(m, z, torch.zeros_like(z))
    az = zm.abs()
    cover = [((az <= k) & m).sum().double() for k in (1, 2, 3)]
    return torch.stack([mask.sum().double(), zm[..., 0].sum(), zm[..., 1].sum(), (zm * zm).sum(), az.sum()] + cover)


def _keypoint_stats(v):
    n = int(v[0])
    if n == 0:
        return dict(count=0, mean_z=[0.0, 0.0], rms_z=0.0, mean_abs_z=0.0, coverage_count=[0, 0, 0],
                    coverage=[0.0, 0.0, 0.0])
    cc = [int(c) for c in v[5:8]]
    return dict(count=n, mean_z=[float(v[1]) / n, float(v[2]) / n], rms_z=math.sqrt(float(v[3]) / (2 * n)),
                mean_abs_z=float(v[4]) / (2 * n), coverage_count=cc, coverage=[c / (2 * n) for c in cc])


def summarize_records(r, sigma_gain=1.0):
    """Calibration.summarize's work on the concatenated records r (tensors on any device: z, kp_flags, nees,
    calib_status, score, pred_score, cov_status): sums, stable sorts and cumulative sums where the tensors
    live, one copy to the host.  -> (what threshold_for needs, the summary dict)."""
    valid = (r["kp_flags"] & 1) != 0
    inl = valid & ((r["kp_flags"] & 2) != 0)
    ok = r["calib_status"] == 0
    nees = torch.where(ok[:, None], r["nees"], torch.zeros_like(r["nees"]))
    below = [((r["nees"][:, c] <= q) & ok).sum().double()
             for c, qs in ((0, CHI2_6), (1, CHI2_3), (2, CHI2_3)) for q in qs]
    head = torch.cat([_keypoint_sums(r["z"], valid), _keypoint_sums(r["z"], inl),
                      torch.stack([ok.sum().double()] + list(nees.sum(0)) + below),
                      torch.stack([(r["calib_status"] == s).sum().double() for s in range(5)])])
    # sparsification: stable descending sorts with the images without a covariance last
    keep = r["cov_status"] == 0
    N = keep.shape[0]
    ninf = torch.full_like(r["score"], -math.inf)
    score = torch.where(keep, r["score"], torch.zeros_like(r["score"]))
    parts = []
    ranks = []
    for key in (torch.where(keep, r["pred_score"], ninf), torch.where(keep, r["score"], ninf)):
        ks, order = torch.sort(key, descending=True, stable=True)
        suffix = torch.flip(torch.cumsum(torch.flip(score[order], (0,)), 0), (0,))
        rank = torch.empty_like(order)
        rank[order] = torch.arange(N, device=order.device)
        ranks.append(rank)
        parts += [ks, suffix]
    d = torch.where(keep, ranks[0] - ranks[1], torch.zeros_like(ranks[0]))
    tail = torch.stack([keep.sum().double(), (d * d).sum().double()])
    flat = torch.cat([head, tail] + [parts[0], parts[1], parts[3]]).cpu().numpy()   # the one synchronisation

    # the layout of `flat`, in the order it was packed above
    fields = iter(flat)
    take = lambda k: [next(fields) for _ in range(k)]
    f_all, f_inl = take(KP_SUMS), take(KP_SUMS)
    (f_n,), f_nees, f_below, f_status = take(1), take(3), take(9), take(5)
    (f_M, f_d2) = take(2)
    arrays = flat[2 * KP_SUMS + 20:]
    assert len(arrays) == 3 * N
    pred_sorted, suf_p, suf_o = (arrays[i * N:(i + 1) * N] for i in range(3))

    g = float(sigma_gain)
    kp_all, kp_inl = _keypoint_stats(f_all), _keypoint_stats(f_inl)
    n = int(f_n)
    mean_nees = [float(x) / n for x in f_nees] if n else [0.0, 0.0, 0.0]
    cnt = [int(x) for x in f_below]
    below = {name: dict(count=cnt[3 * i:3 * i + 3], share=[c / n if n else 0.0 for c in cnt[3 * i:3 * i + 3]])
             for i, name in enumerate(("full", "rot", "trans"))}
    M, d2 = int(f_M), float(f_d2)
    host = (M, pred_sorted[:M].copy(), suf_p[:M].copy())
    fr = [k / STEPS for k in range(STEPS)]
    if M:
        removed = [(k * M) // STEPS for k in range(STEPS)]
        by_pred = [float(suf_p[c]) / (M - c) for c in removed]
        oracle = [float(suf_o[c]) / (M - c) for c in removed]
        mean = float(suf_p[0]) / M
        diff = [a - b for a, b in zip(by_pred, oracle)]
        area = sum(0.5 * (diff[k] + diff[k + 1]) / STEPS for k in range(STEPS - 1))
        sp = dict(count=M, fractions=fr, by_pred=by_pred, oracle=oracle, random=[mean] * STEPS,
                  ause=area / mean if mean > 0 else 0.0,
                  spearman=1.0 - 6.0 * d2 / (M * (M * M - 1)) if M > 1 else 0.0)
    else:
        sp = dict(count=0, fractions=fr, by_pred=[0.0] * STEPS, oracle=[0.0] * STEPS, random=[0.0] * STEPS,
                  ause=0.0, spearman=0.0)
    return host, dict(gain_in_force=g, keypoints=dict(all=kp_all, inliers=kp_inl), sigma_gain=kp_inl["rms_z"] * g,
                pose=dict(count=n, mean_nees=mean_nees, below_chi2=below, cov_gain=math.sqrt(mean_nees[0] / 6.0) * g),
                status_count=[int(x) for x in f_status], sparsification=sp)


class Calibration:
    """Accumulates calibration records and (true score, predicted score) pairs over a validation set on the
    device; update() never synchronises with the host, summarize() does once.  sigma_gain: the calibration
    factor under test (module docstring).  solver: the solver that solves the poses -- its camera matrix and
    landmarks are the records' (calibration_records); None stands for a plain solver with Camera.K and the 11
    SPEED landmarks and refuses poses solved through a lens.  sigma_floor: pose_covariance's, keep them equal.
    Under torch.distributed every rank accumulates and summarises its own images; nothing here gathers."""

    def __init__(self, sigma_gain=1.0, solver=None, sigma_floor=1e-3):
        self.sigma_gain = _check_gain(sigma_gain)
        self.solver = solver
        self.sigma_floor = float(sigma_floor)
        self.batches = []
        self._host = None

    def update(self, points_px, probs, sigmas, poses, cov, q_gt, t_gt, s_t, s_q, clip_bbox=None, stream=None):
        """One batch: the records of calibration_records (cov: pose_covariance's dict at gain 1) and the
        pairs score = s_t + s_q, pred_score * gain, kept as device tensors.  On `stream` (None: the current
        one), where the inputs were made.  -> the batch's records."""
        rec = calibration_records(points_px, probs, sigmas, poses, cov, q_gt, t_gt, clip_bbox=clip_bbox,
                                  sigma_floor=self.sigma_floor, sigma_gain=self.sigma_gain, stream=stream,
                                  solver=self.solver)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            rec = dict(rec, score=(s_t + s_q).double(), pred_score=cov["pred_score"].double() * self.sigma_gain,
                       cov_status=cov["cov_status"].clone())
        self.batches.append((rec, stream))
        self._host = None
        return rec

    def records(self):
        """Everything accumulated, concatenated on the device (on the current stream, after the streams the
        batches were made on)."""
        for _, st in self.batches:
            if st is not None:
                torch.cuda.current_stream().wait_stream(st)
        keys = RECORDS + ("score", "pred_score", "cov_status")
        return {k: torch.cat([r[k] for r, _ in self.batches]) for k in keys}

    def summarize(self):
        """-> a plain dict (python numbers and lists):
        keypoints.all / .inliers   over the valid keypoints (kp_flags bit 0) / those that are also taking-part
                                   inliers: count, mean_z per axis, rms_z, mean_abs_z, coverage_count and
                                   coverage at 1, 2, 3 sigma over the 2 * count axis samples
        sigma_gain                 inliers' rms_z * the gain in force: the gain that would make it 1
        pose                       count of status-0 images, mean_nees (full, rotation, translation),
                                   below_chi2.{full, rot, trans}: count / share at or below the 50 / 90 / 99 %
                                   quantile (6, 3, 3 degrees of freedom), cov_gain = sqrt(mean NEES / 6) * gain
        status_count               images per calib_status 0 .. 4
        sparsification             over the images with cov_status 0: by_pred / oracle / random, the mean true
                                   score left after removing the worst floor(k N / 20), k = 0 .. 19, by predicted
                                   score (descending, then image index), by true score, and in no order; ause, the
                                   trapezoid area between the first two over the removed fraction, over the mean
                                   score; spearman, the rank correlation of the two stable orders
        gain_in_force              this accumulator's sigma_gain"""
        if not self.batches:
            raise ValueError("Calibration.summarize: no batch was added")
        self._host, summary = summarize_records(self.records(), self.sigma_gain)
        return summary

    def threshold_for(self, risk):
        """The largest pred_score threshold t (one of the accumulated, calibrated predicted scores) whose kept
        set {pred_score <= t}, among the images with a covariance, has a mean true score <= risk, and the
        fraction of those images it keeps: (None, 0.0) when no threshold qualifies.  Uses summarize()'s
        download (and runs it when nothing was downloaded yet)."""
        if self._host is None:
            self.summarize()
        M, pred, suffix = self._host
        best = (None, 0.0)
        c = M
        # pred is descending: walk the distinct values upwards; position c is the first image kept
        while c > 0:
            t = pred[c - 1]
            while c > 0 and pred[c - 1] == t:
                c -= 1
            if float(suffix[c]) / (M - c) <= risk:
                best = (float(t), (M - c) / M)
        return best

    def stats_line(self, summary=None):
        s = summary if summary is not None else self.summarize()
        return ("calibration: sigma gain {:.4f}, covariance gain {:.4f}, mean NEES {:.3f} over {:d} poses, "
                "AUSE {:.4f}, Spearman {:.3f}").format(s["sigma_gain"], s["pose"]["cov_gain"], s["pose"]["mean_nees"][0],
                                                       s["pose"]["count"], s["sparsification"]["ause"],
                                                       s["sparsification"]["spearman"])
