"""ORACLE (test infrastructure only -- never imported by the product path).

numpy restatement of the reference's submission-path input pipeline, SpeedSubmission
(REV/datasets/speed.py:44-160), the dataset gen_submission_single.py / gen_submission_multi.py read:

  REV/datasets/speed.py:92-108    generate_clip_bbox: x1 = int(xc - s / 2), y1 = int(yc - s / 2),
                                  side = int(s), s = 1.2 x max side (fp64; int() truncates towards
                                  zero); box = [x1, y1, x1 + side, y1 + side], never clipped
  REV/datasets/speed.py:113-144   __getitem__: a side x side zero canvas with the in-frame part of
                                  the box copied in (the 2020-12-14 "pad instead of squeeze" rule)
  REV/datasets/speed.py:146-153   A.Resize(S, S, cv2.INTER_CUBIC), F.to_tensor, Normalize: the
                                  restatements of oracle/preprocess_ref.py (resize_cubic_u8,
                                  to_tensor_normalize), with their unpinned part (OpenCV itself)

tests/golden/submission_front_ref.npz pins box, canvas and copy to the reference's own code
(scripts/gen_golden_submission.py).

Status rule (decided here, parity UNPINNED): status 1 and zeros when side <= 0 or when the box
shares no positive-area overlap with the frame.  There the reference either raises (an empty
source slice assigned to a non-empty destination) or, through numpy's negative-slice
wrap-around, returns an all-black crop, depending on the side the box lies on.
"""
from __future__ import annotations

import numpy as np

from preprocess_ref import resize_cubic_u8, to_tensor_normalize


def generate_clip_bbox(bbox):
    """REV/datasets/speed.py:92-108, in its operation order."""
    x1, y1, x2, y2 = (float(v) for v in bbox)
    bbox_width, bbox_height = x2 - x1, y2 - y1
    scale = max(bbox_width, bbox_height) * 1.2
    x_center, y_center = (x1 + x2) / 2, (y1 + y2) / 2
    half_scale = scale / 2
    x1, y1 = int(x_center - half_scale), int(y_center - half_scale)
    scale = int(scale)
    return np.asarray([x1, y1, x1 + scale, y1 + scale], np.int64)


def is_empty(clip, width, height):
    """The status rule: no canvas, or no positive-area overlap of the box with the frame."""
    x1, y1, x2, y2 = (int(v) for v in clip)
    return x2 - x1 <= 0 or max(x1, 0) >= min(x2, width) or max(y1, 0) >= min(y2, height)


def pad_crop(img, clip):
    """REV/datasets/speed.py:123-144 for a box that overlaps the frame: img uint8 [H, W] or
    [H, W, C] -> the side x side canvas."""
    height, width = img.shape[:2]
    side = int(clip[2] - clip[0])
    canvas = np.zeros((side, side) + img.shape[2:], img.dtype)
    x1, y1 = max(0, int(clip[0])), max(0, int(clip[1]))
    cx1, cy1 = x1 - int(clip[0]), y1 - int(clip[1])
    x2, y2 = min(width, int(clip[2])), min(height, int(clip[3]))
    canvas[cy1:cy1 + y2 - y1, cx1:cx1 + x2 - x1] = img[y1:y2, x1:x2]
    return canvas


def preprocess(frames, bboxes, size):
    """frames uint8 [B, H, W] (grayscale) or [B, H, W, 3]; bboxes [B, 4] detector boxes.  Returns
    images fp32 [B, 3, S, S], crops uint8 [B, S, S] or [B, S, S, 3] (the resized canvases),
    clip_bbox int64 [B, 4] and status [B] (1: zeros in images and crops)."""
    B, H, W = frames.shape[:3]
    imgs = np.zeros((B, 3, size, size), np.float32)
    crops = np.zeros((B, size, size) + frames.shape[3:], np.uint8)
    clips = np.zeros((B, 4), np.int64)
    status = np.zeros(B, np.int32)
    for i in range(B):
        clips[i] = generate_clip_bbox(bboxes[i])
        if is_empty(clips[i], W, H):
            status[i] = 1
            continue
        crops[i] = resize_cubic_u8(pad_crop(frames[i], clips[i]), size)
        imgs[i] = to_tensor_normalize(crops[i])
    return {"images": imgs, "crops": crops, "clip_bbox": clips, "status": status}
