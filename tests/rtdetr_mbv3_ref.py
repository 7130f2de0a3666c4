"""Torch-fp32 functional restatement of the UNC RT-DETR model behind the MobileNetV3_Large backbone
(UNC/nn/backbone/mobilenetv3.py:28-225), written from the model's definition over the weight dict
(reference state_dict keys).  The backbone feeds oracle/rtdetr_ref.py's hybrid encoder and decoder,
which are imported unchanged.

Points that are easy to miss (all pinned by tests/golden/rtdetr_mbv3l_s256.npz):
  * the stem output is resized to a hard-coded 64 x 64 (bilinear, align_corners=False) before Conv1 /
    Conv2; at a 256 input that is 128 -> 64, exactly a 2 x 2 mean, and only there are the three maps
    the stride 8 / 16 / 32 levels the hybrid encoder needs;
  * in a Block the activation follows the residual add: act3(bn3(conv3(.)) + skip);
  * ReLU in blocks 0-5, Hardswish in blocks 6-14; the SE gate is Hardsigmoid = relu6(x + 3) / 6;
  * the stride-2 skip is depthwise 3x3/2 + BN, then a 1x1 conv WITH bias + BN;
  * linear3 / bn3 are never called.

`rounder` (optional) is applied to every tensor a kernel stores and to every weight it reads: with a
bf16 round trip it models the bf16 model's storage points (used to size the bf16 gates).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import rtdetr_ref
from rtdetr_ref import _t
from spe.rtdetr_spec import MBV3_LARGE_BLOCKS


def _bn(x, w, p):
    return F.batch_norm(x, _t(w, f"{p}.running_mean"), _t(w, f"{p}.running_var"), _t(w, f"{p}.weight"),
                        _t(w, f"{p}.bias"), False, 0.0, 1e-5)


def _fold(w, conv, bn, bias=None, rounder=None):
    """conv weight with its eval BatchNorm folded in (what the kernels read) -> (weight, bias)"""
    cw = _t(w, f"{conv}.weight").double()
    scale = _t(w, f"{bn}.weight").double() / torch.sqrt(_t(w, f"{bn}.running_var").double() + 1e-5)
    shift = _t(w, f"{bn}.bias").double() - _t(w, f"{bn}.running_mean").double() * scale
    if bias is not None:
        shift = shift + _t(w, bias).double() * scale
    cw = (cw * scale.view(-1, 1, 1, 1)).float()
    return (rounder(cw) if rounder else cw), shift.float()


def hardswish(x):
    return x * F.relu6(x + 3.0) / 6.0


def hardsigmoid(x):
    return F.relu6(x + 3.0) / 6.0


def se_module(x, w, p):
    """SeModule (mobilenetv3.py:28-42): pool -> 1x1 -> BN -> ReLU -> 1x1 -> Hardsigmoid, scales x."""
    s = x.mean((2, 3), keepdim=True)
    s = F.relu(_bn(F.conv2d(s, _t(w, f"{p}.se.1.weight")), w, f"{p}.se.2"))
    return x * hardsigmoid(F.conv2d(s, _t(w, f"{p}.se.4.weight")))


def block(x, w, p, k, cin, ce, cout, hs, se, stride, trace=None):
    """Block.forward (mobilenetv3.py:110-120)."""
    act = hardswish if hs else F.relu
    o = act(_bn(F.conv2d(x, _t(w, f"{p}.conv1.weight")), w, f"{p}.bn1"))
    o = act(_bn(F.conv2d(o, _t(w, f"{p}.conv2.weight"), None, stride, k // 2, 1, ce), w, f"{p}.bn2"))
    if se:
        if trace is not None:
            s = o.mean((2, 3), keepdim=True)
            s = F.relu(_bn(F.conv2d(s, _t(w, f"{p}.se.se.1.weight")), w, f"{p}.se.se.2"))
            trace.setdefault("se_pre", {})[p] = F.conv2d(s, _t(w, f"{p}.se.se.4.weight")).flatten()
        o = se_module(o, w, f"{p}.se")
    o = _bn(F.conv2d(o, _t(w, f"{p}.conv3.weight")), w, f"{p}.bn3")
    skip = x
    if stride == 1 and cin != cout:
        skip = _bn(F.conv2d(x, _t(w, f"{p}.skip.0.weight")), w, f"{p}.skip.1")
    elif stride == 2 and cin != cout:
        skip = _bn(F.conv2d(x, _t(w, f"{p}.skip.0.weight"), None, 2, 1, 1, cin), w, f"{p}.skip.1")
        skip = _bn(F.conv2d(skip, _t(w, f"{p}.skip.2.weight"), _t(w, f"{p}.skip.2.bias")), w, f"{p}.skip.3")
    elif stride == 2:
        skip = _bn(F.conv2d(x, _t(w, f"{p}.skip.0.weight"), None, 2, 1, 1, cin), w, f"{p}.skip.1")
    if trace is not None:
        trace.setdefault("pre_act", {})[p] = (o + skip).flatten()
    return act(o + skip)


def mobilenetv3_large(x, w, trace=None):
    """MobileNetV3_Large.forward (mobilenetv3.py:206-225) -> [b, c, out]."""
    b_ = "backbone"
    out = hardswish(_bn(F.conv2d(x, _t(w, f"{b_}.conv1.weight"), None, 2, 1), w, f"{b_}.bn1"))
    b = F.interpolate(out, size=(64, 64), mode="bilinear", align_corners=False)
    b = hardswish(_bn(F.conv2d(b, _t(w, f"{b_}.Conv1.weight"), None, 2, 1), w, f"{b_}.Bn1"))
    c = hardswish(_bn(F.conv2d(b, _t(w, f"{b_}.Conv2.weight"), None, 2, 1), w, f"{b_}.Bn2"))
    for i, (k, cin, ce, cout, hs, se, stride) in enumerate(MBV3_LARGE_BLOCKS):
        out = block(out, w, f"{b_}.bneck.{i}", k, cin, ce, cout, hs, se, stride, trace)
        if trace is not None:
            trace.setdefault("block_out", []).append(out)
    out = hardswish(_bn(F.conv2d(out, _t(w, f"{b_}.conv2.weight")), w, f"{b_}.bn2"))
    return [b, c, out]


def mobilenetv3_large_rounded(x, w, rounder):
    """The same backbone as the HIP model computes it -- BatchNorm folded into the conv weights, the
    2 x 2 mean in front of Conv1 exact, the SE gate in fp32 on the pool of the stored tensor -- with
    `rounder` applied to every weight the MFMA / depthwise kernels read and every tensor they store."""
    b_ = "backbone"
    r = rounder

    def cba(x, conv, bn, act, stride=1, pad=0, groups=1, bias=None, res=None, scale=None):
        cw, cb = _fold(w, conv, bn, bias, r)
        if scale is not None:
            x = r(x * scale)              # the project conv rounds its scaled A operand
        y = F.conv2d(x, cw, cb, stride, pad, 1, groups)
        if res is not None:
            y = y + res
        return r(act(y) if act else y)

    out = cba(x, f"{b_}.conv1", f"{b_}.bn1", hardswish, 2, 1)
    bm = F.avg_pool2d(out, 2)             # folded into Conv1's weights in the model: not stored
    bm = cba(bm, f"{b_}.Conv1", f"{b_}.Bn1", hardswish, 2, 1)
    c = cba(bm, f"{b_}.Conv2", f"{b_}.Bn2", hardswish, 2, 1)
    for i, (k, cin, ce, cout, hs, se, stride) in enumerate(MBV3_LARGE_BLOCKS):
        p = f"{b_}.bneck.{i}"
        act = hardswish if hs else F.relu
        o = cba(out, f"{p}.conv1", f"{p}.bn1", act)
        o = cba(o, f"{p}.conv2", f"{p}.bn2", act, stride, k // 2, ce)
        scale = None
        if se:
            s = o.mean((2, 3), keepdim=True)
            s = F.relu(_bn(F.conv2d(s, _t(w, f"{p}.se.se.1.weight")), w, f"{p}.se.se.2"))
            scale = hardsigmoid(F.conv2d(s, _t(w, f"{p}.se.se.4.weight")))
        skip = out
        if stride == 1 and cin != cout:
            skip = cba(out, f"{p}.skip.0", f"{p}.skip.1", None)
        elif stride == 2:
            skip = cba(out, f"{p}.skip.0", f"{p}.skip.1", None, 2, 1, cin)
            if cin != cout:
                skip = cba(skip, f"{p}.skip.2", f"{p}.skip.3", None, bias=f"{p}.skip.2.bias")
        out = cba(o, f"{p}.conv3", f"{p}.bn3", act, res=skip, scale=scale)
    out = cba(out, f"{b_}.conv2", f"{b_}.bn2", hardswish)
    return [bm, c, out]


@torch.no_grad()
def forward(images, w, cfg, trace=None, backbone=None):
    """images [B, 3, 256, 256] fp32 -> dict of the reference's outputs (as rtdetr_ref.forward)."""
    x = images if torch.is_tensor(images) else torch.from_numpy(images)
    feats = backbone(x.float(), w) if backbone else mobilenetv3_large(x.float(), w, trace)
    enc, aifi = rtdetr_ref.hybrid_encoder(feats, w, cfg)
    if trace is not None:
        trace.update(feats=feats, enc=enc, aifi=aifi)
    return rtdetr_ref.rtdetr_decoder(enc, w, cfg, trace)
