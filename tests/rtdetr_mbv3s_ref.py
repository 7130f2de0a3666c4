"""Torch-fp32 functional restatement of the UNC RT-DETR model behind the MobileNetV3_Small backbone
(UNC/nn/backbone/mobilenetv3.py:228-320), written from the model's definition over the weight dict
(reference state_dict keys), and fp64 references of the fused entry kernel (csrc/mbv3s.hip).  The Block is
tests/rtdetr_mbv3_ref.py's (all three skip forms); the hybrid encoder and decoder are oracle/rtdetr_ref.py's.

What differs from MobileNetV3_Large (all pinned by tests/golden/rtdetr_mbv3s_s256.npz):
  * Conv1 / Conv2 are bare 3x3/s2 convolutions: no BatchNorm, no Hardswish, no bias;
  * block 0 runs on the 128 x 128 x 16 stem map with stride 2, squeeze-excite and in == out, so its skip is
    depthwise 3x3/2 + BatchNorm alone;
  * ReLU in blocks 0-2, Hardswish in blocks 3-10; every block from 3 on has an SE gate;
  * conv2 is 96 -> 512; linear3 (576 -> 1280) / bn3 are never called.

Entry kernel references (fp64, NHWC outputs, any S that is a multiple of 4):
  entry_weights(w)            the kernel's folded fp32 weight buffer [1040] from a model weight dict
  entry_random_weights(seed)  the same buffer drawn directly, with biases large enough that act(bias) != 0
  entry_ref64(x, wbuf)        stem, pooled, skip, expanded, t2 from a normalised batch [B, 3, S, S]
  normalise_crops(u8)         the fp32 batch to_tensor + Normalize make of 8-bit crops, in the kernels' order
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import rtdetr_ref
from rtdetr_ref import _t
from rtdetr_mbv3_ref import _bn, _fold, block, hardsigmoid, hardswish
from spe.rtdetr_spec import MBV3_SMALL_BLOCKS

# offsets into the entry kernel's weight buffer (include/spe.h, spe_debug_mbs_entry)
W_STEM, W_STEM_B, W_EXP, W_EXP_B, W_DW, W_DW_B, W_SKIP, W_SKIP_B, W_FLOATS = 0, 432, 448, 704, 720, 864, 880, 1024, 1040


def mobilenetv3_small(x, w, trace=None):
    """MobileNetV3_Small.forward (mobilenetv3.py:301-320) -> [b, c, out]."""
    b_ = "backbone"
    out = hardswish(_bn(F.conv2d(x, _t(w, f"{b_}.conv1.weight"), None, 2, 1), w, f"{b_}.bn1"))
    if trace is not None:
        trace["stem"] = out
    b = F.interpolate(out, size=(64, 64), mode="bilinear", align_corners=False)
    b = F.conv2d(b, _t(w, f"{b_}.Conv1.weight"), None, 2, 1)
    c = F.conv2d(b, _t(w, f"{b_}.Conv2.weight"), None, 2, 1)
    for i, (k, cin, ce, cout, hs, se, stride) in enumerate(MBV3_SMALL_BLOCKS):
        out = block(out, w, f"{b_}.bneck.{i}", k, cin, ce, cout, hs, se, stride, trace)
        if trace is not None:
            trace.setdefault("block_out", []).append(out)
    out = hardswish(_bn(F.conv2d(out, _t(w, f"{b_}.conv2.weight")), w, f"{b_}.bn2"))
    return [b, c, out]


def mobilenetv3_small_rounded(x, w, rounder, fused=True):
    """The same backbone as the HIP model computes it -- BatchNorm folded into the conv weights, the 2 x 2 mean
    in front of Conv1 exact, the SE gate in fp32 on the pool of the stored tensor -- with `rounder` applied to
    every weight the MFMA / depthwise kernels read and every tensor they store.  fused: the entry kernel's
    storage points (pooled, skip and t2 are the first tensors rounded; its own weights stay fp32); otherwise
    the launch-per-layer path's (the stem map and block 0's expanded tensor are stored too, Conv1 reads the
    stored stem map through the folded 2 x 2 mean)."""
    b_ = "backbone"
    r = rounder

    def cba(x, conv, bn, act, stride=1, pad=0, groups=1, bias=None, res=None, scale=None, rw=True, store=True):
        if bn is None:
            cw, cb = _t(w, f"{conv}.weight"), None
            cw = r(cw) if rw else cw
        else:
            cw, cb = _fold(w, conv, bn, bias, r if rw else None)
        if scale is not None:
            x = r(x * scale)              # the project conv rounds its scaled A operand
        y = F.conv2d(x, cw, cb, stride, pad, 1, groups)
        if res is not None:
            y = y + res
        y = act(y) if act else y
        return r(y) if store else y

    p0 = f"{b_}.bneck.0"
    stem = cba(x, f"{b_}.conv1", f"{b_}.bn1", hardswish, 2, 1, rw=False, store=not fused)
    if fused:
        bm = r(F.avg_pool2d(stem, 2))
        e = cba(stem, f"{p0}.conv1", f"{p0}.bn1", F.relu, rw=False, store=False)
        head = (cba(e, f"{p0}.conv2", f"{p0}.bn2", F.relu, 2, 1, 16, rw=False),
                cba(stem, f"{p0}.skip.0", f"{p0}.skip.1", None, 2, 1, 16, rw=False))
    else:
        bm = F.avg_pool2d(stem, 2)        # folded into Conv1's weights: not stored
        head = None
    bm = cba(bm, f"{b_}.Conv1", None, None, 2, 1)
    c = cba(bm, f"{b_}.Conv2", None, None, 2, 1)
    out = stem
    for i, (k, cin, ce, cout, hs, se, stride) in enumerate(MBV3_SMALL_BLOCKS):
        p = f"{b_}.bneck.{i}"
        act = hardswish if hs else F.relu
        if i == 0 and head is not None:
            o, skip = head
        else:
            o = cba(out, f"{p}.conv1", f"{p}.bn1", act)
            o = cba(o, f"{p}.conv2", f"{p}.bn2", act, stride, k // 2, ce, rw=False)
            skip = out
            if stride == 1 and cin != cout:
                skip = cba(out, f"{p}.skip.0", f"{p}.skip.1", None)
            elif stride == 2:
                skip = cba(out, f"{p}.skip.0", f"{p}.skip.1", None, 2, 1, cin, rw=False)
                if cin != cout:
                    skip = cba(skip, f"{p}.skip.2", f"{p}.skip.3", None, bias=f"{p}.skip.2.bias")
        scale = None
        if se:
            s = o.mean((2, 3), keepdim=True)
            s = F.relu(_bn(F.conv2d(s, _t(w, f"{p}.se.se.1.weight")), w, f"{p}.se.se.2"))
            scale = hardsigmoid(F.conv2d(s, _t(w, f"{p}.se.se.4.weight")))
        out = cba(o, f"{p}.conv3", f"{p}.bn3", act, res=skip, scale=scale)
    out = cba(out, f"{b_}.conv2", f"{b_}.bn2", hardswish)
    return [bm, c, out]


@torch.no_grad()
def forward(images, w, cfg, trace=None, backbone=None):
    """images [B, 3, 256, 256] fp32 -> dict of the reference's outputs (as rtdetr_ref.forward)."""
    x = images if torch.is_tensor(images) else torch.from_numpy(images)
    feats = backbone(x.float(), w) if backbone else mobilenetv3_small(x.float(), w, trace)
    enc, aifi = rtdetr_ref.hybrid_encoder(feats, w, cfg)
    if trace is not None:
        trace.update(feats=feats, enc=enc, aifi=aifi)
    return rtdetr_ref.rtdetr_decoder(enc, w, cfg, trace)


# ---------------------------------------------------------------- the entry kernel
def entry_weights(w):
    """The fused entry's weight buffer (fp32 [1040]) from a model weight dict, BatchNorm folded in double."""
    b_, p = "backbone", "backbone.bneck.0"
    buf = torch.zeros(W_FLOATS, dtype=torch.float32)

    def put(off, boff, conv, bn, layout):
        cw, cb = _fold(w, conv, bn)
        buf[off:off + cw.numel()] = layout(cw).reshape(-1)
        buf[boff:boff + 16] = cb

    put(W_STEM, W_STEM_B, f"{b_}.conv1", f"{b_}.bn1", lambda t: t.reshape(16, 27).t())          # [27][16]
    put(W_EXP, W_EXP_B, f"{p}.conv1", f"{p}.bn1", lambda t: t.reshape(16, 16).t())              # [ci][co]
    put(W_DW, W_DW_B, f"{p}.conv2", f"{p}.bn2", lambda t: t.reshape(16, 9).t())                 # [9][16]
    put(W_SKIP, W_SKIP_B, f"{p}.skip.0", f"{p}.skip.1", lambda t: t.reshape(16, 9).t())
    return buf


def entry_random_weights(seed):
    """A weight buffer drawn directly: He-scaled taps, and shifts of +-(0.5 .. 1.5) on every stage, so
    hswish(stem bias) and relu(expand bias) are far from 0 -- a border padded with act(bias) instead of zero
    moves the outputs by O(0.1 .. 1)."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.zeros(W_FLOATS, dtype=torch.float32)

    def shift():
        return (torch.rand(16, generator=g) + 0.5) * torch.where(torch.rand(16, generator=g) < 0.7, 1.0, -1.0)

    buf[W_STEM:W_STEM + 432] = torch.randn(432, generator=g) * (2.0 / 27) ** 0.5
    buf[W_EXP:W_EXP + 256] = torch.randn(256, generator=g) * (2.0 / 16) ** 0.5
    buf[W_DW:W_DW + 144] = torch.randn(144, generator=g) * (2.0 / 9) ** 0.5
    buf[W_SKIP:W_SKIP + 144] = torch.randn(144, generator=g) * (2.0 / 9) ** 0.5
    for off in (W_STEM_B, W_EXP_B, W_DW_B, W_SKIP_B):
        buf[off:off + 16] = shift()
    return buf


def entry_ref64(x, wbuf):
    """fp64 reference of the entry: x [B, 3, S, S] (any float dtype) -> dict of NHWC fp64 tensors: stem and
    expanded [B, S/2, S/2, 16], pooled / skip / t2 [B, S/4, S/4, 16].  conv2d's zero padding is the
    reference's: the stem map and the expanded map are zero outside the frame."""
    x, wb = x.double(), wbuf.double()
    sw = wb[W_STEM:W_STEM + 432].reshape(27, 16).t().reshape(16, 3, 3, 3)
    stem = F.conv2d(x, sw, wb[W_STEM_B:W_STEM_B + 16], 2, 1)
    stem = stem * F.relu6(stem + 3.0) / 6.0
    ew = wb[W_EXP:W_EXP + 256].reshape(16, 16).t().reshape(16, 16, 1, 1)
    exp = F.relu(F.conv2d(stem, ew, wb[W_EXP_B:W_EXP_B + 16]))
    dw = wb[W_DW:W_DW + 144].reshape(9, 16).t().reshape(16, 1, 3, 3)
    t2 = F.relu(F.conv2d(exp, dw, wb[W_DW_B:W_DW_B + 16], 2, 1, 1, 16))
    kw = wb[W_SKIP:W_SKIP + 144].reshape(9, 16).t().reshape(16, 1, 3, 3)
    skip = F.conv2d(stem, kw, wb[W_SKIP_B:W_SKIP_B + 16], 2, 1, 1, 16)
    pooled = F.avg_pool2d(stem, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    return dict(stem=nhwc(stem), expanded=nhwc(exp), pooled=nhwc(pooled), skip=nhwc(skip), t2=nhwc(t2))


def normalise_crops(u8):
    """8-bit crops [B, S, S] (gray) or [B, S, S, 3] -> the fp32 batch [B, 3, S, S]: (u / 255 - mean) / std with
    fp32 operations in that order (to_tensor + Normalize; a gray byte feeds all three channels)."""
    u = torch.as_tensor(u8)
    if u.dim() == 3:
        u = u.unsqueeze(-1).expand(-1, -1, -1, 3)
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32)
    q = u.to(torch.float32) / torch.tensor(255.0, dtype=torch.float32)
    return ((q - mean) / std).permute(0, 3, 1, 2).contiguous()
