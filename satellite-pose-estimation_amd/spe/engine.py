"""evaluate() with the reference's signature (REV/engine.py:78-135).

Per batch: one device pass (model + fused PostProcess), one batched solver launch and one
D2H copy of the pose records, instead of the reference's per-image Python solver loop.
The criterion (Hungarian matcher + losses, REV/engine.py:99-112) runs on the device
(spe.models.SetCriterion) when given; its losses are logged like the reference's
MetricLogger: per-batch values averaged over batches, weighted ("loss", "loss_ce", ...) and
"<k>_unscaled", plus "class_error".

evaluate_rtdetr() is the UNC RT-DETR model's loop (UNC/solver/speed_engine.py:123-202) over the
same pieces, with spe.rtdetr.SetCriterion and the reference's extra log fields.

generate_submission() is the reference's gen_submission loop (REV/gen_submission_single.py:113-187,
gen_submission_multi.py:123-186) from the JPEG files' bytes to the {filename: pose} log.

What follows the model in the three loops is spe.poststage.PostStage.  A camera with lens distortion comes
with the solver (spe.solver, lens=): the stage hands it the crop's size as the sigmas' scale and everything
downstream reads the undistorted keypoints.
"""
from __future__ import annotations

import io

import numpy as np
import torch

from . import _lib
from . import dist as spe_dist
from .poststage import PostStage
from .speed_eval import SpeedEval, device_speed_score


def _log_losses(ld, weight_dict, device, log):
    """One batch's criterion outputs into the meters like the reference's MetricLogger update
    (REV/engine.py:102-112, UNC/solver/speed_engine.py:157-173): rank-averaged values, "loss" = the
    sum of the weighted ones, "<k>" weighted, "<k>_unscaled" as returned, plus "class_error"."""
    ld = {k: float(v) for k, v in ld.items()}
    if spe_dist.is_dist():                            # utils.reduce_dict (REV/engine.py:103)
        vals = torch.tensor([ld[k] for k in sorted(ld)], dtype=torch.float64, device=device)
        torch.distributed.all_reduce(vals)
        ld = dict(zip(sorted(ld), (vals / torch.distributed.get_world_size()).tolist()))
    scaled = {k: v * weight_dict[k] for k, v in ld.items() if k in weight_dict}
    log("loss", sum(scaled.values()))
    for k, v in scaled.items():
        log(k, v)
    for k, v in ld.items():
        log(k + "_unscaled", v)
    log("class_error", ld["class_error"])


def _evaluate(model, criterion, data_loader, gt_file, solver, device, calibration, sigma_gain, landmarks, *,
              box_areas, self_assess, unc_log, pose_cov):
    """The loop of evaluate() and evaluate_rtdetr().  What the two differ in: box_areas (the Ceres-style solver's
    per-image thresholds from the ground-truth box areas, checked up front), self_assess (run it on a model with
    sigmas), unc_log (the UNC log's three aux_outputs entries) and pose_cov (pred_score / cov_status per record)."""
    evaluator = SpeedEval(gt_file, solver)
    cal = None
    if calibration:
        from .calibration import Calibration
        cal = Calibration(sigma_gain=sigma_gain, solver=solver)
    post = PostStage(solver, self_assess, pose_cov, sigma_gain, cal, landmarks, score=device_speed_score)
    ceres = box_areas and getattr(solver, "mode", None) == _lib.SPE_PNP_EPNP_CERES
    if ceres:
        # EPnPCeresSolver's per-image thresholds come from the ground-truth box areas: refuse up front a
        # ground truth without them (load_ground_truth sets "area" only from bbox_xxyy).  The area-driven
        # threshold itself is parity unpinned: the REV SpeedEval calls the solver without an area
        # (REV/datasets/speed.py:399, commented out); UNC's passes it (speed_dataset.py:396-399).
        missing = [f for f, g in evaluator.ground_truth.items() if "area" not in g]
        if missing:
            raise ValueError(f"EPnPCeresSolver evaluation needs ground-truth box areas (bbox_xxyy); "
                             f"{len(missing)} entries lack them, e.g. {missing[0]}")
    meters = {}

    def log(k, v):
        s = meters.setdefault(k, [0.0, 0])
        s[0] += float(v)
        s[1] += 1

    for samples, targets in data_loader:
        samples = samples.to(device)
        filenames = [t["filename"] for t in targets]
        clip = torch.stack([torch.as_tensor(t["clip_bbox"], dtype=torch.float32) for t in targets]).to(device)
        outputs = model(samples, clip_bbox=clip)
        extra = {}
        if unc_log:
            aux = outputs.get("aux_outputs", [])
            if len(aux) < 3:
                raise ValueError(f"the UNC evaluation log needs three aux_outputs entries, the model returned {len(aux)}")
            extra["aux_logits"] = [a["pred_logits"] for a in aux[:3]]
        if criterion is not None:
            ld = criterion(outputs, [{k: v.to(device) for k, v in t.items() if torch.is_tensor(v)} for t in targets])
            _log_losses(ld, criterion.weight_dict, device, log)
        sig = outputs.get("sigmas")
        if cal is not None and sig is None:
            raise ValueError("evaluate: calibration needs a model with a sigma head")
        gt = [evaluator.ground_truth[f] for f in filenames]
        q_gt = torch.tensor([g["quat"] for g in gt], dtype=torch.float64, device=device)
        t_gt = torch.tensor([g["tvec"] for g in gt], dtype=torch.float64, device=device)
        # EPnPCeresSolver: one threshold per image from its ground-truth box area (UNC SpeedEval
        # passes ground_truth[filename]["area"], src/data/speed/speed_dataset.py:396-399)
        p = post(outputs, clip, q_gt, t_gt, area=[g["area"] for g in gt] if ceres else None)
        evaluator.update_batch(filenames, outputs["points_px"], outputs["probs"], p.poses, p.s_t, p.s_q, sig, p.assess,
                               **extra)
        if p.cov is not None:
            _log_pred_score(evaluator.log, filenames, p.cov)
    evaluator.log = spe_dist.all_gather_log(evaluator.log)
    evaluator.summarize()
    stats = {k: s / max(n, 1) for k, (s, n) in meters.items()}
    if cal is not None:
        # the summary into the returned stats and one line onto the evaluator's
        stats["calibration"] = cal.summarize()
        evaluator.stats += "; " + cal.stats_line(stats["calibration"])
    stats["speed_eval_pose"] = evaluator.stats
    return stats, evaluator


@torch.no_grad()
def evaluate(model, criterion, postprocessors, data_loader, gt_file, solver, device, output_dir=None,
             calibration=False, sigma_gain=1.0, landmarks=None):
    """landmarks (a spe.landmarks.LandmarkReconstruction, None: nothing changes): every batch's keypoints,
    their sigmas and ground-truth poses are added to it (update(), one launch, no synchronisation); the caller
    runs landmarks.solve() afterwards.

    calibration (a model with a sigma head): the keypoint sigmas, the pose covariance and its predicted score are
    compared with the ground truth over the whole set (spe.calibration.Calibration at sigma_gain); the returned
    stats then carry the summary dict under "calibration" and evaluator.stats one more line.  With several ranks
    the log is gathered but the calibration is not: each rank's summary and line cover the images it evaluated."""
    return _evaluate(model, criterion, data_loader, gt_file, solver, device, calibration, sigma_gain, landmarks,
                     box_areas=True, self_assess=True, unc_log=False, pose_cov=False)


@torch.no_grad()
def evaluate_rtdetr(model, criterion, postprocessors, data_loader, gt_file, solver, device, output_dir=None,
                    pose_cov=False, sigma_gain=1.0, calibration=False, landmarks=None):
    """The UNC RT-DETR evaluation loop (UNC/solver/speed_engine.py:123-202) with evaluate()'s
    interface.  Per batch: one device pass (RTDETR.forward with clip_bbox, so RTDETRPostProcessor
    runs fused; `postprocessors` is accepted for the reference's signature), the device criterion
    (spe.rtdetr.SetCriterion), one batched sigma solve and one D2H copy of the pose records.

    The losses are logged exactly as the reference logs them: its criterion returns values already
    multiplied by weight_dict and the loop multiplies the main layer's (the only keys weight_dict
    names) by weight_dict again, so "loss" and "<k>" carry the weight twice and "<k>_unscaled"
    once.  The log entries carry the reference's extra fields (UNC speed_dataset.py:424-438):
    "sigma" and "aux_points_0..2", the first three aux_outputs entries' pred_logits (the reference
    stores logits under that name) rounded to 2 decimals.  pose_cov: each entry also carries
    "pred_score", the pose covariance's first-order prediction of the image's score
    (PoseSolver.pose_covariance; 0 where cov_status is not 0, which "cov_status" tells), computed with
    the sigmas times sigma_gain.  calibration: as for evaluate(); the covariance is computed for it whether
    pose_cov is set or not, and the log entries are those of a run without it.  landmarks: as for evaluate()."""
    return _evaluate(model, criterion, data_loader, gt_file, solver, device, calibration, sigma_gain, landmarks,
                     box_areas=False, self_assess=False, unc_log=True, pose_cov=pose_cov)


def _log_pred_score(log, filenames, cov):
    """pred_score / cov_status of PoseSolver.pose_covariance into the per-image records."""
    ps, cs = cov["pred_score"].cpu().numpy(), cov["cov_status"].cpu().numpy()
    for i, f in enumerate(filenames):
        log[f]["pred_score"] = float(np.around(ps[i], decimals=8))
        log[f]["cov_status"] = int(cs[i])


def _host_decode(data, height, width, filename):
    """Image.open(path).convert('RGB') (REV/datasets/speed.py:116) of one file on the host."""
    from PIL import Image
    rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    if rgb.shape[:2] != (height, width):
        raise ValueError(f"{filename}: a {rgb.shape[1]}x{rgb.shape[0]} frame in a batch of {width}x{height} frames")
    return rgb


def _batch_frames(files, names, decoder, device):
    """JPEG bytes of one batch -> device frames uint8 [B,H,W], or [B,H,W,3] when a frame is not gray.
    The device decoder takes the baseline grayscale files (SPEED's format); a file it refuses
    (status != 0: colour, progressive, oversized) is decoded with Pillow and its frame uploaded."""
    from .datasets import JpegDecoder
    dec = decoder(*JpegDecoder.pack(files, device))
    frames = dec["frames"]
    refused = np.nonzero(dec["status"].cpu().numpy())[0]
    if len(refused) == 0:
        return frames
    H, W = frames.shape[1:3]
    host = {int(i): _host_decode(files[i], H, W, names[i]) for i in refused}
    gray = all((f[..., 0] == f[..., 1]).all() and (f[..., 0] == f[..., 2]).all() for f in host.values())
    if not gray:
        frames = frames[..., None].expand(-1, -1, -1, 3).contiguous()
    for i, f in host.items():
        frames[i] = torch.from_numpy(np.array(f[..., 0] if gray else f)).to(device)
    return frames


@torch.no_grad()
def generate_submission(models, postprocessors, anns, read_file, solver, device, batch_size, input_size,
                        decoder=None, transform=None, pose_cov=False, sigma_gain=1.0):
    """The reference's gen_submission loop (REV/gen_submission_single.py:113-187; with a list of
    models, gen_prediction + gen_submission of gen_submission_multi.py:123-186) over SpeedSubmission
    (REV/datasets/speed.py:44-160), from the files' bytes on.

    anns: the detector's {filename: [[x1, y1, x2, y2, score], ...]} mapping (load_anns, :59-82); the
    first box of each file is used, in the mapping's order.  read_file(filename) -> the JPEG file's
    bytes.  Per batch (the last may be short, drop_last=False): JpegDecoder, SpeedSubmissionTransform
    (u8 crops), the model(s) with the fused PostProcess, one batched solve -- solver.solve_batch, or
    solver.solve_batch_multi for a list of models (Multi_Mean_PoseSolver) -- and one D2H copy of the
    pose records.  Returns {filename: {"quat_pr", "tvec_pr"}}, rounded to 6 decimals like the
    reference; a failed solve (the reference's IndexError / cv2.error) or a status-1 crop gives the
    zero pose.  `postprocessors` is accepted for the reference's signature: PostProcess runs fused
    in the model's forward.  decoder / transform default to JpegDecoder() (SPEED's 1920x1200 frames)
    and SpeedSubmissionTransform(input_size); every frame of a run has the decoder's size.

    A single spe.rtdetr.RTDETR works the same way (UNC's SpeedSubmission, src/data/speed/speed_dataset.py:
    59-168, is this pad-to-square crop): its u8 stems take the crops, its sigmas go to the solver -- a sigma
    solver such as SimplePoseSolverSigma (epnp_ransac_sigma).  A list of RTDETR models takes a
    SigmaEnsemblePoseSolver: every model's sigmas and the batch's clip_bbox go to its solve_batch_multi, which
    fuses them into one keypoint set with a sigma (the reference has no sigma fusion rule; include/spe.h
    spe_ensemble_fuse_sigma defines one) and solves it with its backend; a model without sigmas is a
    ValueError.  Any other ensemble solver is called as solve_batch_multi(points, probs).  Not supported
    here: EPnPCeresSolver, also as an ensemble's backend, whose per-image thresholds the reference derives
    from the ground-truth box areas a submission set does not have (ValueError).

    pose_cov (a single model with a sigma head, or a list with a SigmaEnsemblePoseSolver, whose fused probs
    and sigmas it then reads): each record also carries "pred_score" and "cov_status"
    (PoseSolver.pose_covariance on the crop-scaled sigmas, times sigma_gain, the calibration factor
    spe.calibration measures); a status-1 crop's are 0 and 1, like its pose."""
    from .datasets import JpegDecoder, SpeedSubmissionTransform
    from .solver import SigmaEnsemblePoseSolver
    multi = isinstance(models, (list, tuple))
    if multi and not hasattr(solver, "solve_batch_multi"):
        raise ValueError("a list of models needs an ensemble solver (Multi_Mean_PoseSolver, SigmaEnsemblePoseSolver)")
    if getattr(solver, "mode", None) == _lib.SPE_PNP_EPNP_CERES:
        raise ValueError("generate_submission: EPnPCeresSolver takes one threshold per image from the ground-truth "
                         "box areas (UNC speed_dataset.py:366-399), which a submission set lacks; use a solver "
                         "without them (epnp_ransac_sigma)")
    sigma_multi = multi and isinstance(solver, SigmaEnsemblePoseSolver)
    if pose_cov and multi and not sigma_multi:
        raise ValueError("generate_submission: pose_cov needs a single model's sigmas (no fusion rule for sigmas) "
                         "or a SigmaEnsemblePoseSolver")
    decoder = decoder if decoder is not None else JpegDecoder()
    transform = transform if transform is not None else SpeedSubmissionTransform(input_size)
    post = PostStage(solver, pose_cov=pose_cov, sigma_gain=sigma_gain)
    names = list(anns)
    log = {}
    for i0 in range(0, len(names), int(batch_size)):
        batch = names[i0:i0 + int(batch_size)]
        bbox = np.asarray([anns[f][0][:4] for f in batch], np.float64)
        frames = _batch_frames([read_file(f) for f in batch], batch, decoder, device)
        t = transform(frames, bbox, crops=True, images=False)
        poses = None
        if multi:
            outs = [m(t["crops"], clip_bbox=t["clip_bbox"]) for m in models]
            if sigma_multi:
                if any(o.get("sigmas") is None for o in outs):
                    raise ValueError("generate_submission: SigmaEnsemblePoseSolver needs models with a sigma head")
                poses = solver.solve_batch_multi([o["points_px"] for o in outs], [o["probs"] for o in outs],
                                                 [o["sigmas"] for o in outs], clip_bbox=t["clip_bbox"])
                # what pose_cov reads: the fused keypoint set in one model's layout
                o = {"probs": poses["fused"]["probs"], "sigmas": poses["fused"]["sigmas"]}
            else:
                poses = solver.solve_batch_multi([o["points_px"] for o in outs], [o["probs"] for o in outs])
                o = {}
        else:
            o = models(t["crops"], clip_bbox=t["clip_bbox"])
        if pose_cov and o.get("sigmas") is None:
            raise ValueError("generate_submission: pose_cov needs a model with a sigma head")
        p = post(o, t["clip_bbox"], poses=poses)
        # failed images carry the zero pose, as in SpeedEval.update_batch: every solver status but OK
        # and RANSAC_FALLBACK, and here a status-1 crop too
        st = p.poses["status"]
        failed = ((st != _lib.SPE_PNP_OK) & (st != _lib.SPE_PNP_RANSAC_FALLBACK)) | (t["status"] != 0)
        rec = torch.cat([p.poses["quat"].double(), p.poses["tvec"].double(), failed.double()[:, None]], 1).cpu().numpy()
        for f, r in zip(batch, rec):
            quat, tvec = (np.zeros(4), np.zeros(3)) if r[7] else (r[0:4], r[4:7])
            log[f] = {"quat_pr": np.around(quat, decimals=6).tolist(), "tvec_pr": np.around(tvec, decimals=6).tolist()}
        if p.cov is not None:
            bad, cov = t["status"] != 0, p.cov
            cov["pred_score"] = cov["pred_score"].masked_fill(bad, 0.0)
            cov["cov_status"] = torch.where(bad & (cov["cov_status"] == 0), torch.ones_like(cov["cov_status"]),
                                            cov["cov_status"])
            _log_pred_score(log, batch, cov)
    return log
