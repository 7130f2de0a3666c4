"""Torch-fp32 functional restatement of the UNC RT-DETR model behind the GhostNetV2 backbone
(UNC/nn/backbone/ghostnetv2.py:44-441), written from the model's definition over the weight dict
(reference state_dict keys).  The backbone feeds oracle/rtdetr_ref.py's hybrid encoder and decoder,
which are imported unchanged.

Points that are easy to miss (all pinned by tests/golden/rtdetr_ghostv2_s256.npz):
  * the RAW conv_stem output (no norm, no activation) is resized to a hard-coded 64 x 64 (bilinear,
    align_corners=False) before Conv1 / Conv2; at a 256 input that is 128 -> 64, exactly a 2 x 2 mean;
    relu(bn1(.)) of the same tensor feeds the blocks;
  * a ghost module is cat(x1, cheap(x1)) with x1 = primary(x); in mode "attn" (blocks >= 2, ghost1 only)
    the concat is multiplied by sigmoid(short_conv(avg_pool2(x))) upsampled nearest x2 -- the gate applies
    AFTER the cheap operation, which reads the ungated x1; no activation between the 1x5 and 5x1 convs;
  * ghost2 has no activation, and neither has the block after the residual add;
  * the SE block's two convs carry biases and no norm; its gate is Hardsigmoid = relu6(x + 3) / 6, and the
    tensor it pools is already DFC-gated;
  * the shortcut is depthwise k x k / stride + BN, then 1x1 + BN, whenever in != out or stride 2;
  * conv_head / classifier are never called.

`ghostnetv2_rounded` is the backbone as the HIP model computes it; its `rnd` is applied to every weight
the MFMA kernels read and to every tensor a kernel stores (the depthwise, DFC, SE and stem kernels read
fp32 weights): with a bf16 round trip it models the bf16 model's storage points.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import rtdetr_ref
from rtdetr_ref import _t
from spe.rtdetr_spec import GHOSTV2_BLOCKS, GHOSTV2_ATTN_FROM, ghostv2_block_keys


def _bn(x, w, p):
    return F.batch_norm(x, _t(w, f"{p}.running_mean"), _t(w, f"{p}.running_var"), _t(w, f"{p}.weight"),
                        _t(w, f"{p}.bias"), False, 0.0, 1e-5)


def hardswish(x):
    return x * F.relu6(x + 3.0) / 6.0


def hardsigmoid(x):
    return F.relu6(x + 3.0) / 6.0


def se_pre(x, w, p):
    """SqueezeExcite up to the gate's pre-activation (ghostnetv2.py:63-67)."""
    s = x.mean((2, 3), keepdim=True)
    s = F.relu(F.conv2d(s, _t(w, f"{p}.conv_reduce.weight"), _t(w, f"{p}.conv_reduce.bias")))
    return F.conv2d(s, _t(w, f"{p}.conv_expand.weight"), _t(w, f"{p}.conv_expand.bias"))


def ghost_module(x, w, p, relu, attn, trace=None):
    """GhostModuleV2.forward (ghostnetv2.py:188-201); every width here is even, so out[:, :oup] is the concat."""
    act = F.relu if relu else (lambda t: t)
    x1 = act(_bn(F.conv2d(x, _t(w, f"{p}.primary_conv.0.weight")), w, f"{p}.primary_conv.1"))
    x2 = act(_bn(F.conv2d(x1, _t(w, f"{p}.cheap_operation.0.weight"), None, 1, 1, 1, x1.shape[1]), w,
                 f"{p}.cheap_operation.1"))
    out = torch.cat([x1, x2], 1)
    if not attn:
        return out
    c = out.shape[1]
    r = _bn(F.conv2d(F.avg_pool2d(x, 2, 2), _t(w, f"{p}.short_conv.0.weight")), w, f"{p}.short_conv.1")
    r = _bn(F.conv2d(r, _t(w, f"{p}.short_conv.2.weight"), None, 1, (0, 2), 1, c), w, f"{p}.short_conv.3")
    r = _bn(F.conv2d(r, _t(w, f"{p}.short_conv.4.weight"), None, 1, (2, 0), 1, c), w, f"{p}.short_conv.5")
    if trace is not None:
        trace.setdefault("dfc_pre", {})[p] = r.flatten()
    return out * F.interpolate(torch.sigmoid(r), size=out.shape[-2:], mode="nearest")


def bottleneck(x, w, p, lid, cin, trace=None):
    """GhostBottleneckV2.forward (ghostnetv2.py:273-283)."""
    k, mid, cout, se, stride = GHOSTV2_BLOCKS[lid]
    o = ghost_module(x, w, f"{p}.ghost1", True, lid >= GHOSTV2_ATTN_FROM, trace)
    if stride > 1:
        o = _bn(F.conv2d(o, _t(w, f"{p}.conv_dw.weight"), None, stride, (k - 1) // 2, 1, mid), w, f"{p}.bn_dw")
    if se:
        pre = se_pre(o, w, f"{p}.se")
        if trace is not None:
            trace.setdefault("se_pre", {})[p] = pre.flatten()
        o = o * hardsigmoid(pre)
    o = ghost_module(o, w, f"{p}.ghost2", False, False)
    sc = x
    if not (cin == cout and stride == 1):
        sc = _bn(F.conv2d(x, _t(w, f"{p}.shortcut.0.weight"), None, stride, (k - 1) // 2, 1, cin), w, f"{p}.shortcut.1")
        sc = _bn(F.conv2d(sc, _t(w, f"{p}.shortcut.2.weight")), w, f"{p}.shortcut.3")
    return o + sc


def ghostnetv2(x, w, trace=None):
    """GhostNetV2.forward (ghostnetv2.py:418-441) -> [b, c, out]."""
    b_ = "backbone"
    x = F.conv2d(x, _t(w, f"{b_}.conv_stem.weight"), None, 2, 1)
    b = F.interpolate(x, size=(64, 64), mode="bilinear", align_corners=False)
    b = hardswish(_bn(F.conv2d(b, _t(w, f"{b_}.Conv1.weight"), None, 2, 1), w, f"{b_}.Bn1"))
    c = hardswish(_bn(F.conv2d(b, _t(w, f"{b_}.Conv2.weight"), None, 2, 1), w, f"{b_}.Bn2"))
    x = F.relu(_bn(x, w, f"{b_}.bn1"))
    for lid, p, cin in ghostv2_block_keys():
        x = bottleneck(x, w, p, lid, cin, trace)
        if trace is not None:
            trace.setdefault("block_out", []).append(x)
    x = F.relu(_bn(F.conv2d(x, _t(w, f"{b_}.blocks.9.0.conv.weight")), w, f"{b_}.blocks.9.0.bn1"))
    out = hardswish(_bn(F.conv2d(x, _t(w, f"{b_}.Conv3.weight")), w, f"{b_}.Bn3"))
    return [b, c, out]


def _fold(w, conv, bn):
    """conv weight with its eval BatchNorm folded in, in double -> (weight, bias) fp32"""
    cw = _t(w, f"{conv}.weight").double()
    scale = _t(w, f"{bn}.weight").double() / torch.sqrt(_t(w, f"{bn}.running_var").double() + 1e-5)
    shift = _t(w, f"{bn}.bias").double() - _t(w, f"{bn}.running_mean").double() * scale
    return (cw * scale.view(-1, 1, 1, 1)).float(), shift.float()


def ghostnetv2_rounded(x, w, rnd):
    """The backbone as the HIP model computes it: BatchNorm folded into the weights, the 64 x 64 resize an
    exact 2 x 2 mean of the stored raw stem output, the cheap operation's x2 gated / added before it is
    rounded, the SE gate in fp32 on the pool of the stored tensor and applied to the A operand of ghost2's
    primary conv.  (Channel padding is not modelled: a pad lane holds exactly 0 and meets zero weights.)"""
    b_ = "backbone"
    r = rnd

    def pw(x, conv, bn, act=None, stride=1, pad=0):          # an MFMA conv: rounded weights, rounded output
        cw, cb = _fold(w, conv, bn)
        y = F.conv2d(x, r(cw), cb, stride, pad)
        return r(act(y) if act else y)

    def dw(x, conv, bn, stride=1, pad=1):                    # a depthwise kernel: fp32 weights
        cw, cb = _fold(w, conv, bn)
        return F.conv2d(x, cw, cb, stride, pad, 1, x.shape[1])

    def ghost(x, p, relu, gate=None, res=None, scale=None):
        act = F.relu if relu else None
        if scale is not None:
            x = r(x * scale)
        x1 = pw(x, f"{p}.primary_conv.0", f"{p}.primary_conv.1", act)
        x2 = dw(x1, f"{p}.cheap_operation.0", f"{p}.cheap_operation.1")
        out = torch.cat([x1, F.relu(x2) if relu else x2], 1)
        if gate is not None:
            out = out * F.interpolate(gate, size=out.shape[-2:], mode="nearest")
        if res is not None:
            out = out + res
        return r(out)

    raw = F.conv2d(x, _t(w, f"{b_}.conv_stem.weight"), None, 2, 1)
    bm = pw(F.avg_pool2d(r(raw), 2), f"{b_}.Conv1", f"{b_}.Bn1", hardswish, 2, 1)
    c = pw(bm, f"{b_}.Conv2", f"{b_}.Bn2", hardswish, 2, 1)
    x = r(F.relu(_bn(raw, w, f"{b_}.bn1")))
    for lid, p, cin in ghostv2_block_keys():
        k, mid, cout, se, stride = GHOSTV2_BLOCKS[lid]
        gate = None
        if lid >= GHOSTV2_ATTN_FROM:
            g = f"{p}.ghost1.short_conv"
            t = pw(r(F.avg_pool2d(x, 2)), f"{g}.0", f"{g}.1")
            t = dw(dw(t, f"{g}.2", f"{g}.3", 1, (0, 2)), f"{g}.4", f"{g}.5", 1, (2, 0))
            gate = r(torch.sigmoid(t))
        o = ghost(x, f"{p}.ghost1", True, gate=gate)
        if stride > 1:
            o = r(dw(o, f"{p}.conv_dw", f"{p}.bn_dw", stride, (k - 1) // 2))
        scale = hardsigmoid(se_pre(o, w, f"{p}.se")) if se else None
        sc = x
        if not (cin == cout and stride == 1):
            sc = r(dw(x, f"{p}.shortcut.0", f"{p}.shortcut.1", stride, (k - 1) // 2))
            sc = pw(sc, f"{p}.shortcut.2", f"{p}.shortcut.3")
        x = ghost(o, f"{p}.ghost2", False, res=sc, scale=scale)
    x = pw(x, f"{b_}.blocks.9.0.conv", f"{b_}.blocks.9.0.bn1", F.relu)
    out = pw(x, f"{b_}.Conv3", f"{b_}.Bn3", hardswish)
    return [bm, c, out]


@torch.no_grad()
def forward(images, w, cfg, trace=None, backbone=None):
    """images [B, 3, 256, 256] fp32 -> dict of the reference's outputs (as rtdetr_ref.forward)."""
    x = images if torch.is_tensor(images) else torch.from_numpy(images)
    feats = backbone(x.float(), w) if backbone else ghostnetv2(x.float(), w, trace)
    enc, aifi = rtdetr_ref.hybrid_encoder(feats, w, cfg)
    if trace is not None:
        trace.update(feats=feats, enc=enc, aifi=aifi)
    return rtdetr_ref.rtdetr_decoder(enc, w, cfg, trace)
