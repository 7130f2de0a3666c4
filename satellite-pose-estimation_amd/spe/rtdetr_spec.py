"""Parameter space of the UNC RT-DETR keypoint model.

The reference model is `RTDETR(PResNet, HybridEncoder, RTDETRTransformer)`
(UNC/src/zoo/rtdetr/rtdetr.py:20-38, UNC/nn/backbone/presnet.py:156-265,
UNC/src/zoo/rtdetr/hybrid_encoder.py:196-401, UNC/src/zoo/rtdetr/rtdetr_decoder.py:372-555)
as the speed configs build it (UNC/configs/rtdetr_speed/rtdetr_r{18,50}vd_6x_speed_kl_*.yml:
256x256 input, 30 queries, 3 decoder layers, hybrid-encoder expansion 0.5, no denoising).

* `RtdetrConfig`                 - the config fields those YAML files set.
* `rtdetr_param_shapes(cfg)`     - (key, shape) in the reference's state_dict order
                                   (BatchNorm `num_batches_tracked` buffers omitted, like
                                   FrozenBatchNorm2d drops them, UNC/nn/backbone/common.py:46-68).
* `random_rtdetr_weights(cfg, s)`- deterministic random weights in that key space.
"""
from __future__ import annotations

from dataclasses import dataclass, asdict

import numpy as np

# "MobileNetV3_Small" is spelled as the reference registers the class (`backbone: MobileNetV3_Small` in its
# configs): the lower-case "mobilenetv3_small" is the name tests/test_rtdetr_mbv3.py pins as refused.
BACKBONES = ("presnet", "mobilenetv3_large", "ghostnetv2", "MobileNetV3_Small")
# MobileNetV3_Large.bneck (UNC/nn/backbone/mobilenetv3.py:148-164): kernel, in, expand, out, hardswish, SE, stride
MBV3_LARGE_BLOCKS = [
    (3, 16, 16, 16, False, False, 1), (3, 16, 64, 24, False, False, 2), (3, 24, 72, 24, False, False, 1),
    (5, 24, 72, 40, False, True, 2), (5, 40, 120, 40, False, True, 1), (5, 40, 120, 40, False, True, 1),
    (3, 40, 240, 80, True, False, 2), (3, 80, 200, 80, True, False, 1), (3, 80, 184, 80, True, False, 1),
    (3, 80, 184, 80, True, False, 1), (3, 80, 480, 112, True, True, 1), (3, 112, 672, 112, True, True, 1),
    (5, 112, 672, 160, True, True, 2), (5, 160, 672, 160, True, True, 1), (5, 160, 960, 160, True, True, 1),
]
# MobileNetV3_Small.bneck (mobilenetv3.py:248-260), same columns.  Block 0 is the one row of either table with
# stride 2 and in == out: its skip is depthwise 3x3/2 + BatchNorm alone (the third Block.skip form).
MBV3_SMALL_BLOCKS = [
    (3, 16, 16, 16, False, True, 2), (3, 16, 72, 24, False, False, 2), (3, 24, 88, 24, False, False, 1),
    (5, 24, 96, 40, True, True, 2), (5, 40, 240, 40, True, True, 1), (5, 40, 240, 40, True, True, 1),
    (5, 40, 120, 48, True, True, 1), (5, 48, 144, 48, True, True, 1), (5, 48, 288, 96, True, True, 2),
    (5, 96, 576, 96, True, True, 1), (5, 96, 576, 96, True, True, 1),
]
# GhostNetV2.cfgs at width 1.0 (UNC/nn/backbone/ghostnetv2.py:297-319), one row a block in layer_id order:
# dw kernel, mid (expansion) width, out width, SE ratio, stride.  Blocks 0-1 build ghost1 in mode "original",
# blocks >= 2 in mode "attn" (the DFC branch); the stem and every block's input width chain from 16.
GHOSTV2_BLOCKS = [
    (3, 16, 16, 0, 1), (3, 48, 24, 0, 2), (3, 72, 24, 0, 1), (5, 72, 40, 0.25, 2), (5, 120, 40, 0.25, 1),
    (3, 240, 80, 0, 2), (3, 200, 80, 0, 1), (3, 184, 80, 0, 1), (3, 184, 80, 0, 1), (3, 480, 112, 0.25, 1),
    (3, 672, 112, 0.25, 1), (5, 672, 160, 0.25, 2), (5, 960, 160, 0, 1), (5, 960, 160, 0.25, 1), (5, 960, 160, 0, 1),
    (5, 960, 160, 0.25, 1),
]
GHOSTV2_STAGES = [1, 1, 1, 1, 1, 1, 5, 1, 4]       # blocks per nn.Sequential stage: the key is blocks.{stage}.{j}
GHOSTV2_ATTN_FROM = 2                              # layer_id <= 1: ghost1 mode "original", else "attn"


def ghostv2_se_width(mid):
    """SqueezeExcite's reduced width, _make_divisible(mid * 0.25, 4) (ghostnetv2.py:21-34, 57): 20, 32, 120, 168, 240."""
    v = mid * 0.25
    n = max(4, int(v + 2) // 4 * 4)
    return n + 4 if n < 0.9 * v else n


def ghostv2_block_keys():
    """(layer_id, key prefix, in width) of the 16 blocks."""
    out, cin, lid = [], 16, 0
    for st, n in enumerate(GHOSTV2_STAGES):
        for j in range(n):
            out.append((lid, f"backbone.blocks.{st}.{j}", cin))
            cin = GHOSTV2_BLOCKS[lid][2]
            lid += 1
    return out


RESNET_CFG = {18: [2, 2, 2, 2], 34: [3, 4, 6, 3], 50: [3, 4, 6, 3], 101: [3, 4, 23, 3]}   # presnet.py:17-23


@dataclass(frozen=True)
class RtdetrConfig:
    depth: int = 50                 # PResNet.depth (r18vd / r50vd), variant "d"
    input_size: int = 256           # eval_spatial_size / dataset resize
    num_queries: int = 30           # RTDETRTransformer.num_queries
    dec_layers: int = 3             # RTDETRTransformer.num_decoder_layers
    hidden_dim: int = 256
    nheads: int = 8
    enc_ff: int = 1024              # HybridEncoder.dim_feedforward (AIFI, GELU)
    dec_ff: int = 1024              # RTDETRTransformer.dim_feedforward (ReLU)
    expansion: float = 0.5          # HybridEncoder.expansion (CSPRepLayer hidden = 256 * e)
    num_levels: int = 3
    num_points: int = 4             # num_decoder_points
    num_classes: int = 11           # + 1 no-object logit
    backbone: str = "presnet"       # "presnet" (depth 18 / 50), or "mobilenetv3_large" / "MobileNetV3_Small" / "ghostnetv2" (depth unused, 256 input only)

    def __post_init__(self):
        if self.backbone not in BACKBONES:
            raise ValueError(f"backbone must be one of {BACKBONES}, got {self.backbone!r}")

    @property
    def backbone_channels(self):
        if self.backbone in ("mobilenetv3_large", "MobileNetV3_Small"):
            return [128, 256, 512]                  # Conv1 / Conv2 / conv2 outputs (mobilenetv3.py:215-225, 301-320)
        if self.backbone == "ghostnetv2":
            return [128, 256, 512]                  # Conv1 / Conv2 / Conv3 outputs (ghostnetv2.py:339-341)
        e = 1 if self.depth < 50 else 4
        return [128 * e, 256 * e, 512 * e]          # return_idx [1, 2, 3]: strides 8, 16, 32

    @property
    def level_sizes(self):
        return [self.input_size // s for s in (8, 16, 32)]

    @property
    def tokens(self):
        return sum(s * s for s in self.level_sizes)

    @property
    def csp_hidden(self):
        return int(self.hidden_dim * self.expansion)

    def to_dict(self):
        return asdict(self)


def _bn(p, c):
    return [(f"{p}.{n}", (c,)) for n in ("weight", "bias", "running_mean", "running_var")]


def _cnl(p, cin, cout, k):
    """ConvNormLayer: conv (no bias) + BatchNorm2d (UNC/nn/backbone/common.py:8-25)."""
    return [(f"{p}.conv.weight", (cout, cin, k, k))] + _bn(f"{p}.norm", cout)


def _lin(p, o, i):
    return [(f"{p}.weight", (o, i)), (f"{p}.bias", (o,))]


def _mlp(p, dims):
    out = []
    for j, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        out += _lin(f"{p}.layers.{j}", o, i)
    return out


def _mha(p, d):
    return [(f"{p}.in_proj_weight", (3 * d, d)), (f"{p}.in_proj_bias", (3 * d,))] + _lin(f"{p}.out_proj", d, d)


def _mbv3_block_shapes(b, blocks):
    """The bneck Sequential of either MobileNetV3 (Block.__init__, mobilenetv3.py:48-108)."""
    out = []
    for i, (k, cin, ce, cout, _hs, se, stride) in enumerate(blocks):
        p = f"{b}.bneck.{i}"
        out += [(f"{p}.conv1.weight", (ce, cin, 1, 1))] + _bn(f"{p}.bn1", ce)
        out += [(f"{p}.conv2.weight", (ce, 1, k, k))] + _bn(f"{p}.bn2", ce)
        if se:
            h = max(ce // 4, 8)
            out += [(f"{p}.se.se.1.weight", (h, ce, 1, 1))] + _bn(f"{p}.se.se.2", h)
            out += [(f"{p}.se.se.4.weight", (ce, h, 1, 1))]
        out += [(f"{p}.conv3.weight", (cout, ce, 1, 1))] + _bn(f"{p}.bn3", cout)
        if stride == 1 and cin != cout:
            out += [(f"{p}.skip.0.weight", (cout, cin, 1, 1))] + _bn(f"{p}.skip.1", cout)
        elif stride == 2 and cin != cout:
            out += [(f"{p}.skip.0.weight", (cin, 1, 3, 3))] + _bn(f"{p}.skip.1", cin)
            out += [(f"{p}.skip.2.weight", (cout, cin, 1, 1)), (f"{p}.skip.2.bias", (cout,))] + _bn(f"{p}.skip.3", cout)
        elif stride == 2:
            out += [(f"{p}.skip.0.weight", (cout, 1, 3, 3))] + _bn(f"{p}.skip.1", cout)
    return out


def mbv3_large_param_shapes():
    """MobileNetV3_Large's parameters in registration order (mobilenetv3.py:136-173); linear3 / bn3 are
    built and never called, their keys are part of the state_dict all the same."""
    b = "backbone"
    out = [(f"{b}.conv1.weight", (16, 3, 3, 3))] + _bn(f"{b}.bn1", 16) + _bn(f"{b}.Bn1", 128) + _bn(f"{b}.Bn2", 256)
    out += [(f"{b}.Conv1.weight", (128, 16, 3, 3)), (f"{b}.Conv2.weight", (256, 128, 3, 3))]
    out += _mbv3_block_shapes(b, MBV3_LARGE_BLOCKS)
    out += [(f"{b}.conv2.weight", (512, 160, 1, 1))] + _bn(f"{b}.bn2", 512)
    out += [(f"{b}.linear3.weight", (1280, 960))] + _bn(f"{b}.bn3", 1280)
    return out


def mbv3_small_param_shapes():
    """MobileNetV3_Small's parameters in registration order (mobilenetv3.py:241-270): conv1, the bare Conv1 /
    Conv2 (no BatchNorm of their own), bn1, bneck, conv2, bn2; linear3 / bn3 are built and never called, their
    keys are part of the state_dict all the same."""
    b = "backbone"
    out = [(f"{b}.conv1.weight", (16, 3, 3, 3)), (f"{b}.Conv1.weight", (128, 16, 3, 3)),
           (f"{b}.Conv2.weight", (256, 128, 3, 3))] + _bn(f"{b}.bn1", 16)
    out += _mbv3_block_shapes(b, MBV3_SMALL_BLOCKS)
    out += [(f"{b}.conv2.weight", (512, 96, 1, 1))] + _bn(f"{b}.bn2", 512)
    out += [(f"{b}.linear3.weight", (1280, 576))] + _bn(f"{b}.bn3", 1280)
    return out


def _ghost_module(p, cin, cout, attn):
    """GhostModuleV2 (ghostnetv2.py:88-186): primary 1x1 to ceil(cout / 2), cheap depthwise 3x3 on it, and in
    mode "attn" short_conv = 1x1 + BN, depthwise 1x5 + BN, depthwise 5x1 + BN at full width."""
    h = -(-cout // 2)
    out = [(f"{p}.primary_conv.0.weight", (h, cin, 1, 1))] + _bn(f"{p}.primary_conv.1", h)
    out += [(f"{p}.cheap_operation.0.weight", (h, 1, 3, 3))] + _bn(f"{p}.cheap_operation.1", h)
    if attn:
        out += [(f"{p}.short_conv.0.weight", (cout, cin, 1, 1))] + _bn(f"{p}.short_conv.1", cout)
        out += [(f"{p}.short_conv.2.weight", (cout, 1, 1, 5))] + _bn(f"{p}.short_conv.3", cout)
        out += [(f"{p}.short_conv.4.weight", (cout, 1, 5, 1))] + _bn(f"{p}.short_conv.5", cout)
    return out


def ghostv2_param_shapes():
    """GhostNetV2's parameters in registration order (ghostnetv2.py:331-387); conv_head and classifier are
    built and never called, their keys are part of the state_dict all the same."""
    b = "backbone"
    out = _bn(f"{b}.Bn1", 128) + _bn(f"{b}.Bn2", 256) + _bn(f"{b}.Bn3", 512)
    out += [(f"{b}.Conv1.weight", (128, 16, 3, 3)), (f"{b}.Conv2.weight", (256, 128, 3, 3)),
            (f"{b}.Conv3.weight", (512, 960, 1, 1)), (f"{b}.conv_stem.weight", (16, 3, 3, 3))] + _bn(f"{b}.bn1", 16)
    for lid, p, cin in ghostv2_block_keys():
        k, mid, cout, se, stride = GHOSTV2_BLOCKS[lid]
        out += _ghost_module(f"{p}.ghost1", cin, mid, lid >= GHOSTV2_ATTN_FROM)
        if stride > 1:
            out += [(f"{p}.conv_dw.weight", (mid, 1, k, k))] + _bn(f"{p}.bn_dw", mid)
        if se:
            r = ghostv2_se_width(mid)
            out += [(f"{p}.se.conv_reduce.weight", (r, mid, 1, 1)), (f"{p}.se.conv_reduce.bias", (r,)),
                    (f"{p}.se.conv_expand.weight", (mid, r, 1, 1)), (f"{p}.se.conv_expand.bias", (mid,))]
        out += _ghost_module(f"{p}.ghost2", mid, cout, False)
        if not (cin == cout and stride == 1):
            out += [(f"{p}.shortcut.0.weight", (cin, 1, k, k))] + _bn(f"{p}.shortcut.1", cin)
            out += [(f"{p}.shortcut.2.weight", (cout, cin, 1, 1))] + _bn(f"{p}.shortcut.3", cout)
    out += [(f"{b}.blocks.9.0.conv.weight", (960, 160, 1, 1))] + _bn(f"{b}.blocks.9.0.bn1", 960)
    out += [(f"{b}.conv_head.weight", (1280, 960, 1, 1)), (f"{b}.conv_head.bias", (1280,))]
    out += _lin(f"{b}.classifier", 1000, 1280)
    return out


def rtdetr_param_shapes(cfg: RtdetrConfig):
    d, C = cfg.hidden_dim, cfg.num_classes + 1
    out = [("temper_param", (1,))]
    if cfg.backbone == "mobilenetv3_large":
        out += mbv3_large_param_shapes()
    elif cfg.backbone == "ghostnetv2":
        out += ghostv2_param_shapes()
    elif cfg.backbone == "MobileNetV3_Small":
        out += mbv3_small_param_shapes()
    else:
        out += _presnet_param_shapes(cfg)
    out += _rtdetr_tail_shapes(cfg, d, C)
    return out


def _presnet_param_shapes(cfg):
    # ---- backbone: PResNet variant d (presnet.py:156-230)
    out = _cnl("backbone.conv1.conv1_1", 3, 32, 3) + _cnl("backbone.conv1.conv1_2", 32, 32, 3)
    out += _cnl("backbone.conv1.conv1_3", 32, 64, 3)
    bottleneck = cfg.depth >= 50
    exp = 4 if bottleneck else 1
    cin = 64
    for i, (cout, n) in enumerate(zip([64, 128, 256, 512], RESNET_CFG[cfg.depth])):
        for j in range(n):
            p = f"backbone.res_layers.{i}.blocks.{j}"
            stride = 2 if j == 0 and i > 0 else 1
            blk = []
            if j == 0:                       # shortcut=False on the first block of a stage
                sp = f"{p}.short.conv" if stride == 2 else f"{p}.short"   # variant d: pool + conv
                blk_short = _cnl(sp, cin, cout * exp, 1)
            if bottleneck:
                blk += _cnl(f"{p}.branch2a", cin, cout, 1) + _cnl(f"{p}.branch2b", cout, cout, 3)
                blk += _cnl(f"{p}.branch2c", cout, cout * exp, 1)
                out += blk + (blk_short if j == 0 else [])
            else:                            # BasicBlock registers `short` first (presnet.py:38-53)
                blk += _cnl(f"{p}.branch2a", cin, cout, 3) + _cnl(f"{p}.branch2b", cout, cout, 3)
                out += (blk_short if j == 0 else []) + blk
            cin = cout * exp
    return out


def _rtdetr_tail_shapes(cfg, d, C):
    out = []
    # ---- decoder (RTDETRTransformer, rtdetr_decoder.py:372-505), registered before the encoder
    for lv in range(cfg.num_levels):
        out += _cnl(f"decoder.input_proj.{lv}", d, d, 1)
    P = cfg.nheads * cfg.num_levels * cfg.num_points
    for i in range(cfg.dec_layers):
        p = f"decoder.decoder.layers.{i}"
        out += _mha(f"{p}.self_attn", d) + [(f"{p}.norm1.weight", (d,)), (f"{p}.norm1.bias", (d,))]
        out += _lin(f"{p}.cross_attn.sampling_offsets", 2 * P, d) + _lin(f"{p}.cross_attn.attention_weights", P, d)
        out += _lin(f"{p}.cross_attn.value_proj", d, d) + _lin(f"{p}.cross_attn.output_proj", d, d)
        out += [(f"{p}.norm2.weight", (d,)), (f"{p}.norm2.bias", (d,))]
        out += _lin(f"{p}.linear1", cfg.dec_ff, d) + _lin(f"{p}.linear2", d, cfg.dec_ff)
        out += [(f"{p}.norm3.weight", (d,)), (f"{p}.norm3.bias", (d,))]
    for i in range(cfg.dec_layers):
        out += _mlp(f"decoder.decoder.sigma_embed.{i}", [d, d, d, 1])
    out += _mlp("decoder.query_pos_head", [2, 2 * d, d])
    out += _lin("decoder.enc_output.0", d, d) + [("decoder.enc_output.1.weight", (d,)), ("decoder.enc_output.1.bias", (d,))]
    out += _lin("decoder.enc_score_head", C, d) + _mlp("decoder.enc_bbox_head", [d, d, d, 2])
    for i in range(cfg.dec_layers):
        out += _lin(f"decoder.dec_score_head.{i}", C, d)
    for i in range(cfg.dec_layers):
        out += _mlp(f"decoder.dec_bbox_head.{i}", [d, d, d, 2])
    # ---- hybrid encoder (hybrid_encoder.py:196-300)
    for lv, c in enumerate(cfg.backbone_channels):
        out += [(f"encoder.input_proj.{lv}.0.weight", (d, c, 1, 1))] + _bn(f"encoder.input_proj.{lv}.1", d)
    out += [("encoder.encoder_fusion_input.weight", (d, 3 * d, 1, 1))]       # built, never called
    p = "encoder.encoder.0.layers.0"
    out += _mha(f"{p}.self_attn", d) + _lin(f"{p}.linear1", cfg.enc_ff, d) + _lin(f"{p}.linear2", d, cfg.enc_ff)
    out += [(f"{p}.norm1.weight", (d,)), (f"{p}.norm1.bias", (d,)), (f"{p}.norm2.weight", (d,)), (f"{p}.norm2.bias", (d,))]
    for i in range(cfg.num_levels - 1):
        out += _cnl(f"encoder.lateral_convs.{i}", d, d, 1)
    h = cfg.csp_hidden
    for blocks in ("fpn_blocks", "pan_blocks"):
        for i in range(cfg.num_levels - 1):
            p = f"encoder.{blocks}.{i}"
            out += _cnl(f"{p}.conv1", 2 * d, h, 1) + _cnl(f"{p}.conv2", 2 * d, h, 1)
            out += _cnl(f"{p}.bottlenecks.0.conv1", h, h, 3) + _cnl(f"{p}.bottlenecks.0.conv2", h, h, 1)
            if h != d:
                out += _cnl(f"{p}.conv3", h, d, 1)
    return out


def _draw_mbv3(rng, key, shape, hs_from=6):
    """One MobileNetV3 backbone parameter (hs_from: the first Hardswish block, 6 Large / 3 Small): He-normal
    convs (depthwise: fan-in k*k), non-trivial BatchNorm statistics, the projection norm bn3 damped (gain 0.3) so the residual stream stays O(1)
    through 15 blocks, norms in front of a Hardswish widened (gain 0.75 .. 1.5) so its inputs reach
    past -3 and 3, the SE gate's first conv halved and its second doubled so most gate pre-activations
    stay in (-3, 3) while a few saturate."""
    if key.endswith("running_mean"):
        return rng.normal(0.0, 0.1, shape)
    if key.endswith("running_var"):
        return rng.uniform(0.5, 1.5, shape)
    if len(shape) == 4:
        a = rng.normal(0.0, np.sqrt(2.0 / (shape[1] * shape[2] * shape[3])), shape)
        return a * 0.5 if ".se.se.1." in key else a * 2.0 if ".se.se.4." in key else a
    if len(shape) == 2:
        lim = np.sqrt(6.0 / (shape[0] + shape[1]))
        return rng.uniform(-lim, lim, shape)
    if ".skip.2.bias" in key:
        return rng.normal(0.0, 0.02, shape)
    if key.endswith("weight"):
        part = key.split(".")
        blk = int(part[2]) if part[1] == "bneck" else None
        name = part[-2]
        if blk is not None and name == "bn3":
            return 0.3 * rng.uniform(0.5, 1.0, shape)
        hswish = (blk is None and name in ("bn1", "Bn1", "Bn2", "bn2")) or \
                 (blk is not None and blk >= hs_from and name in ("bn1", "bn2"))
        return rng.uniform(0.75, 1.5, shape) if hswish else rng.uniform(0.5, 1.0, shape)
    return rng.normal(0.0, 0.05, shape)


def _draw_mbv3s(rng, key, shape):
    """One MobileNetV3_Small backbone parameter.  _draw_mbv3's gains let the activations decay through these 11
    blocks (|x| <= 0.1 behind block 10: two Hardswishes of small inputs halve the expanded tensor, every block
    from 3 on has an SE gate near 0.5, most blocks have no identity skip), so: Hardswish norms (bn1 / bn2 of
    blocks >= 3) widened to gain 1.5 .. 3, bn3 gain 0.4 x (0.5 .. 1), the SE gate's second conv tripled.  The
    golden generator's report then shows block output maxima of 0.6 .. 8.5 and up to 32 % saturated gates."""
    a = _draw_mbv3(rng, key, shape, hs_from=3)
    if len(shape) == 4 and ".se.se.4." in key:
        return a * 1.5
    part = key.split(".")
    if len(shape) == 1 and key.endswith("weight") and part[1] == "bneck":
        if part[-2] == "bn3":
            return a * (0.4 / 0.3)
        if int(part[2]) >= 3 and part[-2] in ("bn1", "bn2"):
            return a * 2.0
    return a


GH_RES_GAIN = 0.6     # gain of ghost2's norms and of the shortcut's last norm (see _draw_ghostv2)


def _draw_ghostv2(rng, key, shape):
    """One GhostNetV2 backbone parameter: He-normal convs (depthwise: fan-in k*k), non-trivial BatchNorm
    statistics.  ghost2 has no activation in front of the residual add, so its two norms are damped (gain
    GH_RES_GAIN) to keep the residual stream O(1-10) through 16 blocks, and so is the shortcut's last norm.
    The DFC branch's last norm is widened so the sigmoid's pre-activations reach its saturated ends while
    most stay in its linear region; the SE convs carry biases, the second conv is doubled and its bias
    spread so the Hardsigmoid's pre-activations lie on both sides of -3 and 3."""
    if key.endswith("running_mean"):
        return rng.normal(0.0, 0.1, shape)
    if key.endswith("running_var"):
        return rng.uniform(0.5, 1.5, shape)
    if len(shape) == 4:
        a = rng.normal(0.0, np.sqrt(2.0 / (shape[1] * shape[2] * shape[3])), shape)
        return a * 2.0 if ".se.conv_expand." in key else a
    if len(shape) == 2:
        lim = np.sqrt(6.0 / (shape[0] + shape[1]))
        return rng.uniform(-lim, lim, shape)
    if ".se.conv_reduce.bias" in key:
        return rng.normal(0.0, 0.1, shape)
    if ".se.conv_expand.bias" in key:
        return rng.normal(0.0, 1.5, shape)
    if key.endswith("weight"):
        if ".ghost2." in key or ".shortcut.3." in key:
            return GH_RES_GAIN * rng.uniform(0.5, 1.0, shape)
        if ".short_conv.5." in key:
            return rng.uniform(2.0, 4.0, shape)
        if key.split(".")[1] in ("Bn1", "Bn2", "Bn3"):
            return rng.uniform(0.75, 1.5, shape)
        return rng.uniform(0.5, 1.0, shape)
    if ".short_conv.5." in key:
        return rng.normal(0.0, 0.5, shape)
    return rng.normal(0.0, 0.05, shape)


def random_rtdetr_weights(cfg: RtdetrConfig, seed: int = 0):
    """Deterministic random weights (key -> float32 ndarray) that exercise every path: He-normal
    convs with non-trivial BatchNorm statistics (residual gains damped so activations stay O(1)
    through the bottlenecks), Xavier linears, random sampling offsets (sample points fall inside
    and outside the value maps) and attention logits, non-zero box/sigma heads."""
    rng = np.random.Generator(np.random.PCG64(seed))
    w = {}
    mbv3 = cfg.backbone == "mobilenetv3_large"
    for key, shape in rtdetr_param_shapes(cfg):
        if mbv3 and key.startswith("backbone."):
            a = _draw_mbv3(rng, key, shape)
        elif cfg.backbone == "MobileNetV3_Small" and key.startswith("backbone."):
            a = _draw_mbv3s(rng, key, shape)
        elif cfg.backbone == "ghostnetv2" and key.startswith("backbone."):
            a = _draw_ghostv2(rng, key, shape)
        elif key.endswith("running_mean"):
            a = rng.normal(0.0, 0.1, shape)
        elif key.endswith("running_var"):
            a = rng.uniform(0.5, 1.5, shape)
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            a = rng.normal(0.0, np.sqrt(2.0 / fan_in), shape)
        elif len(shape) == 2:
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            a = rng.uniform(-lim, lim, shape)
            if "sampling_offsets" in key:
                a = a * 4.0
        elif key == "temper_param":
            a = rng.normal(0.0, 1.0, shape)
        else:   # 1-D: BN / LN affine or a bias
            if ".norm." in key or key.startswith("encoder.input_proj") and key.endswith((".1.weight", ".1.bias")):
                if key.endswith("weight"):
                    gain = 0.3 if ("branch2c" in key or "branch2b" in key and cfg.depth < 50) else 1.0
                    a = gain * rng.uniform(0.5, 1.0, shape)
                else:
                    a = rng.normal(0.0, 0.05, shape)
            elif "norm" in key and key.endswith("weight") or key == "decoder.enc_output.1.weight":
                a = 1.0 + rng.normal(0.0, 0.1, shape)
            elif "sampling_offsets" in key:
                a = rng.normal(0.0, 2.0, shape)
            else:
                a = rng.normal(0.0, 0.02, shape)
        w[key] = np.ascontiguousarray(a, dtype=np.float32)
    return w
