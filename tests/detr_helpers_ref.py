"""Plain restatements of the DETR stem, neck and head helper kernels (csrc/elementwise.hip: pack_input,
pack_input_pad4, maxpool3s2, upsample2x, layernorm; csrc/heads.hip: heads, postprocess), written out index by index
rather than through torch's own operators.  tests/test_gpu_detr_helpers.py runs the kernels against them;
tests/test_detr_helpers_ref.py ties them to torch's operators and to oracle/model_ref.py on the CPU.  Test
infrastructure only.

Maps are NHWC, as the kernels store them.  Every function computes in the dtype of the tensors it is given (fp64 for
a reference, fp32 to measure what fp32 arithmetic loses); the pack functions are exact restatements in fp32.
"""
import numpy as np
import torch

# torchvision's ImageNet normalisation, the constants of SrcU8 in elementwise.hip
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


# ---------------------------------------------------------------- pack_input / pack_input_pad4
def normalize_u8(crops):
    """uint8 [B][S][S][channels] (1: gray, feeding all three channels; 3) -> float32 [B][S][S][3]: to_tensor
    (u / 255) then Normalize ((x - mean) / std), every step a rounded numpy float32 operation."""
    crops = np.asarray(crops)
    assert crops.dtype == np.uint8 and crops.shape[-1] in (1, 3)
    u = np.broadcast_to(crops, crops.shape[:-1] + (3,)).astype(np.float32)
    return ((u / np.float32(255.0) - MEAN) / STD).astype(np.float32)


def nchw_to_nhwc(images):
    """float32 [B][3][S][S] -> [B][S][S][3], the values untouched."""
    return torch.as_tensor(images).permute(0, 2, 3, 1).contiguous()


def pack(x3, cpad, dtype=torch.float32):
    """float32 [B][S][S][3] -> dtype [B][S][S][cpad]: the three channels rounded to dtype, the rest +0."""
    x3 = torch.as_tensor(x3)
    out = torch.zeros(x3.shape[:-1] + (cpad,), dtype=dtype)
    out[..., :3] = x3.to(dtype)
    return out


def pack_pad4(x3):
    """float32 [B][S][S][3] -> bf16 [B][S + 6][S + 6][4]: the image inside a 3-pixel border of zeros, channel 3 zero."""
    x3 = torch.as_tensor(x3)
    B, S = x3.shape[:2]
    out = torch.zeros(B, S + 6, S + 6, 4, dtype=torch.bfloat16)
    out[:, 3:3 + S, 3:3 + S, :3] = x3.to(torch.bfloat16)
    return out


# ---------------------------------------------------------------- maxpool3s2
def maxpool3s2(x):
    """[B][H][W][C] -> [B][Ho][Wo][C], Ho = (H - 1) // 2 + 1: the max over rows 2 oh - 1 .. 2 oh + 1 and columns
    2 ow - 1 .. 2 ow + 1 that lie on the map (a pad of -inf)."""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.full((B, Ho, Wo, C), float("-inf"), dtype=x.dtype)
    for oh in range(Ho):
        for ow in range(Wo):
            win = x[:, max(2 * oh - 1, 0):min(2 * oh + 2, H), max(2 * ow - 1, 0):min(2 * ow + 2, W)]
            out[:, oh, ow] = win.reshape(B, -1, C).max(1).values
    return out


# ---------------------------------------------------------------- upsample2x
def _lerp_axis(n_in, dtype):
    """align_corners=True source of each of the 2 n_in outputs along one axis: (index below, index above, weight of
    the one above); src = dst * (n_in - 1) / (2 n_in - 1)."""
    n_out = 2 * n_in
    dst = torch.arange(n_out, dtype=dtype)
    src = dst * (n_in - 1) / (n_out - 1) if n_out > 1 else torch.zeros(n_out, dtype=dtype)
    i0 = src.floor().long().clamp(0, n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, src - i0.to(dtype)


def upsample2x(x):
    """[B][H][W][C] -> [B][2H][2W][C], bilinear with align_corners=True (nn.UpsamplingBilinear2d)."""
    B, H, W, C = x.shape
    y0, y1, ly = _lerp_axis(H, x.dtype)
    x0, x1, lx = _lerp_axis(W, x.dtype)
    ly, lx = ly.reshape(1, -1, 1, 1), lx.reshape(1, 1, -1, 1)
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


# ---------------------------------------------------------------- heads / postprocess
def _mlp3(x, w, p):
    h = torch.relu(x @ w[p + "_w0"].t() + w[p + "_b0"])
    h = torch.relu(h @ w[p + "_w1"].t() + w[p + "_b1"])
    return h @ w[p + "_w2"].t() + w[p + "_b2"]


def softmax(logits):
    e = torch.exp(logits - logits.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def rescale(points, clip_bbox, Q):
    """points [rows][2] in the crop's unit square -> image pixels by the box (x0, y0, x1, y1) of image row // Q."""
    bb = clip_bbox[torch.arange(points.shape[0]) // Q]
    return points * (bb[:, 2:4] - bb[:, 0:2]) + bb[:, 0:2]


def postprocess(logits, points, clip_bbox, Q):
    return {"probs": softmax(logits), "points_px": rescale(points, clip_bbox, Q)}


def heads(hs, w, Q, clip_bbox=None):
    """hs [rows][256]; w: weights as torch stores them ([out][in]): cls_w [12][256], cls_b, pt_w0 / pt_w1 [256][256],
    pt_w2 [2][256] with pt_b*, and optionally sg_* with sg_w2 [1][256].  -> logits, probs, points (sigmoid), points_px
    (with clip_bbox [B][4]), log_sigmas and sigmas (the one column repeated to two)."""
    o = {"logits": hs @ w["cls_w"].t() + w["cls_b"]}
    o["probs"] = softmax(o["logits"])
    o["points"] = 1 / (1 + torch.exp(-_mlp3(hs, w, "pt")))
    if clip_bbox is not None:
        o["points_px"] = rescale(o["points"], clip_bbox, Q)
    if "sg_w0" in w:
        o["log_sigmas"] = _mlp3(hs, w, "sg").repeat(1, 2)
        o["sigmas"] = torch.exp(o["log_sigmas"])
    return o


# ---------------------------------------------------------------- layernorm
def layernorm(x, gamma, beta, eps=1e-5):
    """Rows of x normalised by their mean and the (biased) variance about that mean: two passes."""
    mean = x.sum(-1, keepdim=True) / x.shape[-1]
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / x.shape[-1]
    return d / torch.sqrt(var + eps) * gamma + beta
