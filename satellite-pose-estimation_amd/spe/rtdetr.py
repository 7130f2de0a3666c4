"""Host-side mirror of the UNC RT-DETR keypoint model's inference interface over
the HIP path in libspe.so:

    model = build_rtdetr(RtdetrConfig(depth=50))      # RTDETR(PResNet, HybridEncoder, RTDETRTransformer)
    model.load_state_dict(checkpoint["model"])         # the reference's state_dict keys
    out = model(images)                                # pred_logits / pred_pts / pred_sigmas (+ aux_outputs)
    results = RTDETRPostProcessor()(out, clip_bbox)    # [{logits, points, sigmas}] numpy, per image

Reference: UNC/src/zoo/rtdetr/rtdetr.py:20-53 (RTDETR.forward), rtdetr_decoder.py:672-710 (the
output dict in eval: the last layer's pred_logits / pred_pts / pred_sigmas and aux_outputs =
earlier decoder layers + the encoder top-k), rtdetr_postprocessor.py:44-76.  Every forward runs
the hand-written HIP kernels through the C ABI; there is no torch/CPU compute fallback.
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _lib
from ._hipmodel import HipModel
from .rtdetr_spec import RtdetrConfig, rtdetr_param_shapes, random_rtdetr_weights  # noqa: F401


class RTDETR(HipModel):
    """RTDETR(PResNet-vd | MobileNetV3_Large | MobileNetV3_Small | GhostNetV2, HybridEncoder, RTDETRTransformer)
    with the sigma head, eval forward; cfg.backbone picks the backbone ("mobilenetv3_large", "MobileNetV3_Small",
    "ghostnetv2": input_size 256 only).
    dtype "bf16": bf16 storage / MFMA with fp32 accumulation, LayerNorm, softmax and heads;
    "fp32": exact-f32 MFMA everywhere (parity path)."""

    _NAME = "RTDETR"
    _HOST_INPUT = "RTDETR (HIP) expects device tensors"
    _STAGES = "spe_rtdetr_forward_stages"

    def __init__(self, cfg: RtdetrConfig, dtype: str = "bf16", aux_outputs: bool = True):
        super().__init__()
        self.cfg, self.dtype, self.aux_outputs = cfg, dtype, aux_outputs
        self.num_queries = cfg.num_queries
        selector = {"mobilenetv3_large": _lib.SPE_RTDETR_MBV3_LARGE, "MobileNetV3_Small": _lib.SPE_RTDETR_MBV3_SMALL,
                    "ghostnetv2": _lib.SPE_RTDETR_GHOSTNETV2}.get(cfg.backbone, cfg.depth)
        c = _lib.RtdetrConfig(selector, cfg.input_size, cfg.num_queries, cfg.dec_layers, cfg.enc_ff, cfg.dec_ff,
                              cfg.csp_hidden, cfg.num_classes,
                              _lib.SPE_DTYPE_BF16 if dtype == "bf16" else _lib.SPE_DTYPE_F32)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().spe_rtdetr_create(ctypes.byref(c), ctypes.byref(h)), "spe_rtdetr_create")
        self._adopt(h)

    def encode(self, images, ws, stream=None, part=None, B=None):
        """Encode stage (backbone + HybridEncoder): images -> the three level outputs kept in `ws`.
        part="backbone": the backbone alone (images -> the stride 8 / 16 / 32 maps in `ws`);
        part="transformer": the HybridEncoder over the maps a backbone part left in `ws` (images may be
        None, B given).  images: the fp32 batch [B,3,S,S] or 8-bit crops (forward's forms), on the device."""
        self._require_ready("encode")
        stage = {None: _lib.SPE_STAGE_ENCODE, "backbone": _lib.SPE_STAGE_BACKBONE,
                 "transformer": _lib.SPE_STAGE_TRANSFORMER}[part]
        B = images.shape[0] if images is not None else int(B)
        self._run(images, B, ws, stream, None, stage)

    def decode(self, B, ws, clip_bbox=None, stream=None, aux=None, return_hs=False):
        """Decode stage (RTDETRTransformer, heads, fused RTDETRPostProcessor) of the level outputs an
        encode() left in `ws`; returns forward's dict."""
        self._require_ready("decode")
        out, o = self._outputs(B, ws.device, self._clip(clip_bbox, ws.device), self.aux_outputs if aux is None else aux,
                               return_hs)
        self._run(None, B, ws, stream, o, _lib.SPE_STAGE_DECODE)
        return out

    def _outputs(self, B, dev, clip_bbox, aux, return_hs):
        """The output dict of one forward (tensors the call fills) and the C struct over it; clip_bbox:
        fp32, contiguous, on `dev` (the caller keeps it alive over the call)."""
        Q, C = self.cfg.num_queries, self.cfg.num_classes + 1
        f = dict(device=dev)
        out = {"pred_logits": torch.empty(B, Q, C, **f), "pred_pts": torch.empty(B, Q, 2, **f),
               "pred_sigmas": torch.empty(B, Q, 2, **f)}
        if clip_bbox is not None:
            out.update(probs=torch.empty(B, Q, C, **f), points_px=torch.empty(B, Q, 2, **f),
                       sigmas=torch.empty(B, Q, 2, **f))
        nl = self.cfg.dec_layers - 1
        if aux:
            al, ap, asg = torch.empty(nl, B, Q, C, **f), torch.empty(nl, B, Q, 2, **f), torch.empty(nl, B, Q, 2, **f)
            el, ep = torch.empty(B, Q, C, **f), torch.empty(B, Q, 2, **f)
            topk = torch.empty(B, Q, dtype=torch.int32, device=dev)
        else:
            al = ap = asg = el = ep = topk = None
        if return_hs:
            out["hs"] = torch.empty(B, Q, 256, **f)
        o = _lib.RtdetrOutputs(_lib.ptr(out["pred_logits"]), _lib.ptr(out["pred_pts"]), _lib.ptr(out["pred_sigmas"]),
                               _lib.ptr(clip_bbox), _lib.ptr(out.get("probs")), _lib.ptr(out.get("points_px")),
                               _lib.ptr(out.get("sigmas")), _lib.ptr(al), _lib.ptr(ap), _lib.ptr(asg), _lib.ptr(el),
                               _lib.ptr(ep), _lib.ptr(topk), _lib.ptr(out.get("hs")))
        if aux:   # rtdetr_decoder.py:680-700: decoder layers first, the encoder top-k last
            out["aux_outputs"] = [{"pred_logits": al[i], "pred_pts": ap[i], "pred_sigmas": asg[i]} for i in range(nl)]
            out["aux_outputs"].append({"pred_logits": el, "pred_pts": ep})
            out["topk"] = topk
        return out, o

    def forward(self, samples, clip_bbox=None, stream=None, aux=None, return_hs=False):
        """rtdetr.py:36-53 in eval.  Returns pred_logits [B,Q,C+1], pred_pts [B,Q,2], pred_sigmas
        [B,Q,2] (raw) and, with aux, the reference's aux_outputs list.  Passing `clip_bbox`
        ([B,4] device) also runs the fused RTDETRPostProcessor: probs, points_px, sigmas.
        return_hs adds "hs" [B,Q,256], the last decoder layer's output (the heads' input).
        A contiguous device uint8 tensor [B,S,S] (grayscale) or [B,S,S,3] (RGB) is taken as the 8-bit
        crops to_tensor + Normalize would make the batch from (spe_rtdetr_forward_stages_u8):
        bit-identical to the fp32 batch normalised that way."""
        if torch.is_tensor(samples) and samples.dtype == torch.uint8:
            self._crop_channels(samples)              # (a malformed crop batch is refused whatever the model's state)
        self._require_ready("forward")
        images = self._unwrap(samples)
        if images.dtype != torch.uint8:
            images = self._fp32_batch(images)
        else:
            self._crop_channels(images)
        B, dev = images.shape[0], images.device
        out, o = self._outputs(B, dev, self._clip(clip_bbox, dev), self.aux_outputs if aux is None else aux, return_hs)
        self._run(images, B, self.workspace(B, dev, stream), stream, o, _lib.SPE_STAGE_ENCODE | _lib.SPE_STAGE_DECODE)
        return out

    def forward_with_attention(self, samples, dec_layer=-1, clip_bbox=None, stream=None, enc=True, points=True):
        """forward() plus where the model looked (spe_rtdetr_forward_attention).  Returns (out, maps): `out` is
        forward()'s dict, bit for bit; `maps` holds device fp32 tensors
          "enc_map"     [B,T5,T5], T5 = (S/32)^2: the AIFI layer's self-attention averaged over the heads (row =
                        query token; attention_maps.encoder_heatmaps_at with feat = S/32); enc=False skips it
          "dec_map"     [B,Q,L]: the weight query q's deformable cross-attention of decoder layer `dec_layer` puts
                        on each memory token, averaged over the heads; tokens level-major (stride 8, 16, 32), row-major
                        inside a level (attention_maps.rtdetr_decoder_heatmaps).  Rows sum to <= 1: samples that
                        fall off a level read zeros
          "dec_points"  [B,Q,8,3,4,2] the sampling locations (x, y), crop-normalised, and
          "dec_weights" [B,Q,8,3,4] their softmaxed weights; points=False skips both
        and "level_sizes", the side of each level's map.  Negative dec_layer counts from the end.  fp32 batches
        only (the u8 crop form is forward()'s)."""
        self._require_ready("forward_with_attention")
        images = self._fp32_batch(self._unwrap(samples))
        B, dev = images.shape[0], images.device
        out, o = self._outputs(B, dev, self._clip(clip_bbox, dev), self.aux_outputs, False)
        sizes = list(self.cfg.level_sizes)
        Q, T5, L = self.cfg.num_queries, sizes[-1] ** 2, sum(s * s for s in sizes)
        maps = {"dec_map": torch.empty(B, Q, L, device=dev)}
        if enc:
            maps["enc_map"] = torch.empty(B, T5, T5, device=dev)
        if points:
            maps["dec_points"] = torch.empty(B, Q, 8, len(sizes), 4, 2, device=dev)
            maps["dec_weights"] = torch.empty(B, Q, 8, len(sizes), 4, device=dev)
        ws = self.workspace(B, dev, stream)
        _lib.check(_lib.lib().spe_rtdetr_forward_attention(
            self._h, _lib.stream_ptr(stream), _lib.ptr(images), B, _lib.ptr(ws), ws.numel(), ctypes.byref(o),
            int(dec_layer), _lib.ptr(maps.get("enc_map")), _lib.ptr(maps["dec_map"]), _lib.ptr(maps.get("dec_points")),
            _lib.ptr(maps.get("dec_weights"))), "spe_rtdetr_forward_attention")
        maps["level_sizes"] = sizes
        return out, maps

    def backbone_features(self, images, stream=None):
        """The backbone stage alone (spe_debug_rtdetr_backbone): the stride 8 / 16 / 32 maps as fp32 NCHW."""
        self._require_ready("backbone_features")
        images = images.contiguous().float()
        B, dev = images.shape[0], images.device
        feats = [torch.empty(B, ch, s, s, device=dev) for ch, s in zip(self.cfg.backbone_channels, self.cfg.level_sizes)]
        ws = self.workspace(B, dev, stream)
        _lib.check(_lib.lib().spe_debug_rtdetr_backbone(self._h, _lib.stream_ptr(stream), _lib.ptr(images), B, _lib.ptr(ws),
                                                        ws.numel(), *[_lib.ptr(f) for f in feats]),
                   "spe_debug_rtdetr_backbone")
        return feats


class RTDETRPostProcessor(nn.Module):
    """UNC/src/zoo/rtdetr/rtdetr_postprocessor.py:44-76: softmax probabilities, crop ->
    image pixels, sigma = exp(pred_sigmas); returns numpy dicts per image like the reference.
    When the forward already ran the fused post-process (clip_bbox given) its device results are
    reused."""

    def __init__(self, num_classes=11, use_focal_loss=False, num_top_queries=30, remap_mscoco_category=False):
        super().__init__()
        self.num_classes, self.num_top_queries = num_classes, num_top_queries

    @torch.no_grad()
    def forward(self, outputs, clip_bbox):
        if "probs" in outputs:
            prob, pts, sig = outputs["probs"], outputs["points_px"], outputs["sigmas"]
        else:
            prob = torch.softmax(outputs["pred_logits"], -1)
            cb = torch.stack([torch.as_tensor(b, dtype=torch.float32) for b in clip_bbox]).to(prob.device)
            pts = outputs["pred_pts"].clone()
            pts[..., 0] = pts[..., 0] * (cb[:, 2:3] - cb[:, 0:1]) + cb[:, 0:1]
            pts[..., 1] = pts[..., 1] * (cb[:, 3:4] - cb[:, 1:2]) + cb[:, 1:2]
            sig = torch.exp(outputs["pred_sigmas"])
        prob, pts, sig = prob.cpu().numpy(), pts.cpu().numpy(), sig.cpu().numpy()
        return [{"logits": prob[i], "points": pts[i], "sigmas": sig[i]} for i in range(prob.shape[0])]


class SetCriterion(nn.Module):
    """UNC/src/zoo/rtdetr/rtdetr_criterion.py:49-337 with the HungarianMatcher of matcher.py:20-117,
    on the device (spe_criterion_sigma, csrc/criterion_sigma.hip): one call matches and scores the
    main output, every aux decoder layer and the encoder top-k entry (which has no sigma).

    matcher_weight_dict: cost_class / cost_bbox (a cost_giou entry, which the reference requires and
    never uses, is ignored); use_focal_loss is the flag the speed configs share with the matcher
    (include/rtdetr_r50vd.yml:60): the matching cost takes sigmoid(logit) instead of the softmax.
    losses: "labels", "cardinality", "points", "points_uncert" (both point forms write loss_bbox,
    the later entry wins, as in the reference's dict update).  forward returns the reference's dict
    of 0-d device tensors: every loss already multiplied by weight_dict, keys outside weight_dict
    dropped except the main layer's class_error, aux layer i under "<key>_aux_{i}".  The matching
    of the last call is kept in `last_match` ([L,B,T] query per target; layer 0 = main output)."""

    LOSSES = ("labels", "cardinality", "points", "points_uncert")

    def __init__(self, matcher_weight_dict=None, weight_dict=None, losses=("labels", "points_uncert"),
                 eos_coef: float = 1e-4, num_classes: int = 11, use_focal_loss: bool = True):
        super().__init__()
        m = {"cost_class": 2, "cost_bbox": 5} if matcher_weight_dict is None else matcher_weight_dict
        self.cost_class, self.cost_bbox = float(m["cost_class"]), float(m["cost_bbox"])
        self.weight_dict = {"loss_ce": 1, "loss_bbox": 2} if weight_dict is None else dict(weight_dict)
        for name in losses:
            if name not in self.LOSSES:
                raise ValueError(f"unsupported loss {name!r}: the device criterion computes {self.LOSSES}")
        self.losses = tuple(losses)
        self.eos_coef, self.num_classes, self.use_focal_loss = float(eos_coef), int(num_classes), bool(use_focal_loss)
        self.last_match = None
        self._flags = {}

    def _layer_flags(self, flags, dev):
        t = self._flags.get((dev, flags))
        if t is None:
            t = self._flags[(dev, flags)] = torch.tensor(flags, dtype=torch.int32, device=dev)
        return t

    def _layer_dict(self, row, log):
        """One layer's unweighted entries in the reference's order of insertion."""
        d = {}
        for name in self.losses:
            if name == "labels":
                d["loss_ce"] = row[0]
                if log:
                    d["class_error"] = row[1]
            elif name == "cardinality":
                d["cardinality_error"] = row[2]
            elif name == "points":
                d["loss_bbox"] = row[3]
            else:
                d["points_different"] = row[5]
                d["loss_bbox"] = row[4]
        return d

    @torch.no_grad()
    def forward(self, outputs, targets, stream=None):
        layers = [outputs] + list(outputs.get("aux_outputs", []))
        logits = torch.stack([o["pred_logits"] for o in layers]).float().contiguous()
        points = torch.stack([o["pred_pts"] for o in layers]).float().contiguous()
        L, B, Q, C = logits.shape
        if C != self.num_classes + 1:
            raise ValueError(f"pred_logits has {C} classes, the criterion was built for {self.num_classes} + no-object")
        dev = logits.device
        flags = tuple(int("pred_sigmas" in o) for o in layers)
        sig = None
        if any(flags):
            zero = torch.zeros(B, Q, 2, device=dev)
            sig = torch.stack([o["pred_sigmas"].float() if f else zero for o, f in zip(layers, flags)]).contiguous()
        labels = torch.stack([t["labels"] for t in targets]).to(dev, torch.int32).contiguous()
        tpts = torch.stack([t["landmarks"] for t in targets]).to(dev, torch.float32).contiguous()
        T = labels.shape[1]
        num_boxes = float(B * T)                          # rtdetr_criterion.py:293: no clamp, no rank average
        match = torch.empty(L, B, T, dtype=torch.int32, device=dev)
        res = torch.empty(L, 6, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().spe_criterion_sigma(
            _lib.stream_ptr(stream), _lib.ptr(logits), _lib.ptr(points), _lib.ptr(sig),
            _lib.ptr(self._layer_flags(flags, dev)), _lib.ptr(labels), _lib.ptr(tpts), L, B, Q, C, T, self.cost_class,
            self.cost_bbox, int(self.use_focal_loss), self.eos_coef, num_boxes, _lib.ptr(match), _lib.ptr(res)),
            "spe_criterion_sigma")
        self.last_match = match
        wd = self.weight_dict
        losses = {}
        for l in range(L):
            d = self._layer_dict(res[l], log=l == 0)
            sfx = "" if l == 0 else f"_aux_{l - 1}"
            if "class_error" in d:
                losses["class_error"] = d["class_error"]
            losses.update({k + sfx: v * wd[k] for k, v in d.items() if k in wd})
        return losses


def build_rtdetr(cfg: RtdetrConfig = None, dtype: str = "bf16"):
    """(model, postprocessor) of a speed config (UNC/configs/rtdetr_speed/*.yml fields)."""
    cfg = cfg or RtdetrConfig()
    return RTDETR(cfg, dtype), RTDETRPostProcessor(cfg.num_classes, num_top_queries=cfg.num_queries)


def build_rtdetr_criterion(cfg: RtdetrConfig = None, losses=("labels", "points_uncert")):
    """The SetCriterion of a speed config (UNC/configs/rtdetr_speed/rtdetr_r{18,50}vd_6x_speed_kl_*.yml:
    matcher cost_class 2 / cost_bbox 5 with the shared use_focal_loss, loss_ce 1, loss_bbox 2 for
    r18 and 5 for r50; the plain speed_*.yml configs use losses=("labels", "points"))."""
    cfg = cfg or RtdetrConfig()
    return SetCriterion({"cost_class": 2, "cost_bbox": 5}, {"loss_ce": 1, "loss_bbox": 5 if cfg.depth == 50 else 2},
                        losses, eos_coef=1e-4, num_classes=cfg.num_classes, use_focal_loss=True)
