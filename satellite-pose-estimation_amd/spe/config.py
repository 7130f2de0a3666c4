"""Model / camera configuration for the keypoint-set pose path.

Mirrors the argparse fields the reference's `build_model(args)` reads
(REV/main.py:90-187) and the camera constants of REV/utils/utils.py:30-46.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, asdict

import numpy as np

_DATA = os.path.join(os.path.dirname(__file__), "data")


BACKBONES = ("resnet50s8", "resnet50")
NORMS = ("frozen_bn", "group_bn")


@dataclass(frozen=True)
class SpeConfig:
    input_size: int = 416          # --input_size (REV/main.py:99)
    num_queries: int = 11          # --num_queries (REV/main.py:137)
    enc_layers: int = 6            # --enc_layers (REV/main.py:122)
    dec_layers: int = 6            # --dec_layers (REV/main.py:124)
    hidden_dim: int = 256          # --hidden_dim (REV/main.py:130)
    nheads: int = 8                # --nheads (REV/main.py:135)
    dim_feedforward: int = 2048    # --dim_feedforward (REV/main.py:127)
    num_classes: int = 11          # REV/models/detr_speed.py:305 (+1 no-object)
    sigma_head: bool = False       # UNC sigma head (UNC/src/zoo/rtdetr/rtdetr_decoder.py:295-297)
    backbone: str = "resnet50s8"   # --backbone (REV/main.py): "resnet50s8" (Backbone8s) or "resnet50" (Backbone)
    pre_norm: bool = False         # --pre_norm (REV/main.py): normalize_before of both transformer layer classes
    norm: str = "frozen_bn"        # --bn (REV/main.py:118): the backbone's norm layer, "frozen_bn" or "group_bn"

    def __post_init__(self):
        if self.backbone not in BACKBONES:
            raise ValueError(f"backbone {self.backbone!r}: one of {BACKBONES}")
        if self.norm not in NORMS:
            raise ValueError(f"norm {self.norm!r}: one of {NORMS}")

    @property
    def stride(self) -> int:
        # Backbone8s: the stride-8 fusion neck (REV/models/backbone.py:140-142); Backbone: ResNet-50 cut
        # after layer3, stride 16, no neck (REV/models/backbone.py:57-102)
        return 16 if self.backbone == "resnet50" else 8

    @property
    def feat_size(self) -> int:
        return self.input_size // self.stride

    @property
    def tokens(self) -> int:
        return self.feat_size * self.feat_size

    @classmethod
    def from_args(cls, args) -> "SpeConfig":
        """Build from a reference-style argparse.Namespace (REV/main.py:90-187).  The backbone follows
        build_backbone (REV/models/backbone.py:188-195): "resnet50" is the plain stride-16 Backbone, every
        other name the stride-8 Backbone8s -- except resnet18 / resnet34, which the reference cannot run.
        args.bn (REV/models/backbone.py:173-181): "frozen_bn", "bn" and "sync_bn" all map to norm "frozen_bn" -- in
        eval each is the same per-channel affine of its running statistics, eps 1e-5, over the same keys;
        "group_bn" (nn.GroupNorm(32, C), no running statistics) maps to "group_bn"."""
        bn = str(getattr(args, "bn", "frozen_bn"))
        if bn not in ("frozen_bn", "bn", "sync_bn", "group_bn"):
            raise ValueError(f"bn {bn!r}: one of frozen_bn, bn, sync_bn, group_bn")
        name = str(getattr(args, "backbone", "resnet50s8"))
        if name in ("resnet18", "resnet34"):
            raise ValueError(f"backbone {name!r}: the reference declares num_channels 512 for it but returns "
                             "layer3's 256 channels, so its input_proj mismatches (REV/models/backbone.py:71,100); "
                             "not supported")
        return cls(backbone="resnet50" if name == "resnet50" else "resnet50s8",
                   input_size=int(getattr(args, "input_size", 416)),
                   num_queries=int(getattr(args, "num_queries", 11)),
                   enc_layers=int(getattr(args, "enc_layers", 6)),
                   dec_layers=int(getattr(args, "dec_layers", 6)),
                   hidden_dim=int(getattr(args, "hidden_dim", 256)),
                   nheads=int(getattr(args, "nheads", 8)),
                   dim_feedforward=int(getattr(args, "dim_feedforward", 2048)),
                   sigma_head=bool(getattr(args, "sigma_head", False)),
                   pre_norm=bool(getattr(args, "pre_norm", False)),
                   norm="group_bn" if bn == "group_bn" else "frozen_bn")

    def to_dict(self):
        return asdict(self)


class Camera:
    """SPEED camera (REV/utils/utils.py:30-46): fx = 0.0176 m / 5.86e-6 m/px."""
    fx = 0.0176
    fy = 0.0176
    nu = 1920
    nv = 1200
    ppx = 5.86e-6
    ppy = ppx
    fpx = fx / ppx
    fpy = fy / ppy
    K = np.array([[fpx, 0, nu / 2], [0, fpy, nv / 2], [0, 0, 1]], dtype=np.float64)
    dist = np.zeros(5)


@dataclass(frozen=True, eq=False)
class LensModel:
    """A camera with lens distortion: K and OpenCV's coefficients dist = (k1, k2, p1, p2, k3), what the
    reference hands to cv2 as Camera.K / Camera.dist (UNC/utils/speed_eval_ceres.py).  Four coefficients
    are (k1, k2, p1, p2) with k3 = 0.  iters: the rounds of the fixed-point undistortion
    (include/spe.h spe_undistort_points; 5 is cv2.undistortPoints' default criterion).  A solver built
    with lens= undistorts its keypoints and their sigmas on the device before it solves (spe.solver)."""
    K: np.ndarray = None
    dist: np.ndarray = None
    iters: int = 5

    def __post_init__(self):
        K = np.array(Camera.K if self.K is None else self.K, dtype=np.float64)
        d = np.zeros(5) if self.dist is None else np.array(self.dist, dtype=np.float64).ravel()
        if K.shape != (3, 3):
            raise ValueError(f"K must be 3x3, got {K.shape}")
        if d.size not in (4, 5):
            raise ValueError(f"dist takes 4 (k1, k2, p1, p2) or 5 (+ k3) coefficients, got {d.size}")
        if not 1 <= int(self.iters) <= 64:
            raise ValueError(f"iters must be in [1, 64], got {self.iters}")
        d = np.concatenate([d, np.zeros(5 - d.size)])
        K.setflags(write=False)
        d.setflags(write=False)
        object.__setattr__(self, "K", K)
        object.__setattr__(self, "dist", d)
        object.__setattr__(self, "iters", int(self.iters))

    @classmethod
    def from_args(cls, args) -> "LensModel":
        """From a reference-style argparse.Namespace: args.dist (4 or 5 coefficients) when present,
        zero distortion otherwise."""
        return cls(dist=getattr(args, "dist", None))


def world_points() -> np.ndarray:
    """The 11 satellite landmarks (REV/all_result.json 'pt', REV/utils/speed_eval.py:33-39)."""
    with open(os.path.join(_DATA, "world_points.json")) as f:
        return np.asarray(json.load(f)["points"], dtype=np.float64)


def load_world(world=None) -> np.ndarray:
    """A landmark table [L,3] fp64, 1 <= L <= 16, from what a solver's world= takes: None (the packaged
    world_points()), a path to a JSON file in world_points.json's layout ({"points": ...}), an array, or an
    object with .points (spe.landmarks.LandmarkModel)."""
    if world is None:
        return world_points()
    if isinstance(world, (str, os.PathLike)):
        with open(world) as f:
            world = json.load(f)["points"]
    w = np.array(getattr(world, "points", world), dtype=np.float64)
    if w.ndim != 2 or w.shape[1] != 3 or not 1 <= w.shape[0] <= 16 or not np.isfinite(w).all():
        raise ValueError(f"a landmark table is [L,3] finite numbers with 1 <= L <= 16, got shape {w.shape}")
    return w


def quat_to_matrix(q) -> np.ndarray:
    """Rotation matrix of a (w, x, y, z) quaternion, `mathutils.Quaternion(q).to_matrix()`
    convention (used by REV/utils/utils.py:49-53 to project landmarks)."""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def project(pts, q, t, K=None, dist=None) -> np.ndarray:
    """Pinhole projection K [R|t] X (REV/utils/utils.py:56-69).  dist (k1, k2, p1, p2[, k3]): the
    normalised point goes through OpenCV's distortion model first (the distort map of include/spe.h
    spe_distort_points), as cv2.projectPoints does with distCoeffs."""
    K = Camera.K if K is None else K
    R = quat_to_matrix(q)
    pc = np.asarray(pts, np.float64) @ R.T + np.asarray(t, np.float64).reshape(1, 3)
    if dist is not None:
        k1, k2, p1, p2, k3 = LensModel(K, dist).dist
        x, y = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
        r2 = x * x + y * y
        rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        return np.stack((K[0][0] * xd + K[0][2], K[1][1] * yd + K[1][2]), 1)
    uv = pc @ K.T
    return uv[:, :2] / uv[:, 2:3]
