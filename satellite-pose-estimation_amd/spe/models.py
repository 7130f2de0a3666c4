"""Host-side mirror of the reference model interface (REV/models/__init__.py:5-6,
REV/models/detr_speed.py:32-100,264-336) over the HIP path in libspe.so.

    model, criterion, postprocessors = build_model(args)
    model.load_state_dict(state_dict)      # the reference's 412 keys (checkpoint['model']; 408 for --backbone resnet50;
                                           # 326 / 322 for --bn group_bn, whose norms have no running statistics)
    out = model(samples)                   # NestedTensor | list[Tensor] | Tensor [B,3,S,S]
    results = postprocessors['points'](out, clip_bbox_list)

Every forward runs the hand-written HIP kernels through the C ABI; there is no torch/CPU
compute fallback.  torch is only used for device memory and the current stream.
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _lib
from .config import SpeConfig
from ._hipmodel import HipModel


class DETR(HipModel):
    """Keypoint-set predictor (REV/models/detr_speed.py:32-100), HIP implementation.  cfg.backbone
    "resnet50s8": the stride-8 fusion neck (Backbone8s); "resnet50": ResNet-50 cut after layer3 with
    input_proj straight on the stride-16 map (Backbone, REV/models/backbone.py:57-102).  cfg.norm "group_bn":
    nn.GroupNorm(32, C) in the backbone's 43 norm positions (--bn group_bn), computed per image on the device.

    dtype "bf16": bf16 storage / MFMA with fp32 accumulation, softmax, LayerNorm and heads
    (throughput path).  dtype "fp32": exact-f32 MFMA everywhere (parity path).  dtype "fp32x3":
    the fp32 model with split-bf16 MFMA compute (every fp32 operand x = hi + lo in bf16, products
    hi.hi + hi.lo + lo.hi, fp32 accumulation; fast parity path).  dtype "fp32x6": the accuracy-contract
    mode -- fp32x3's attention, every GEMM / convolution at near-fp32 precision (three-way split,
    six products).  dtype "fp32h3": fp32x6 with the backbone / encoder GEMMs and
    convolutions as three fp16 MFMAs on a power-of-two-scaled two-way fp16 split (the same
    near-fp32 products at half fp32x6's MFMAs).
    attn_dtype "fp16" (bf16 models): the encoder self-attention's q/k/V operands are stored
    and multiplied in fp16 (BASELINE config 5, "fp16 MFMA attention")."""

    _NAME = "DETR"
    _HOST_INPUT = "DETR (HIP) expects device tensors; call samples.to('cuda')"
    _STAGES = "spe_forward_stages"

    def __init__(self, cfg: SpeConfig, dtype: str = "bf16", aux_loss: bool = False, attn_dtype: str = None):
        super().__init__()
        self.cfg = cfg
        self.num_queries = cfg.num_queries
        self.aux_loss = aux_loss
        self.dtype = dtype
        if attn_dtype not in (None, dtype, "fp16") or (attn_dtype == "fp16" and dtype != "bf16"):
            raise ValueError(f"attn_dtype {attn_dtype!r}: None, the model dtype, or 'fp16' for bf16 models")
        self.attn_dtype = attn_dtype or dtype
        L = _lib.lib()
        c = _lib.ModelConfig(cfg.input_size, cfg.num_queries, cfg.enc_layers, cfg.dec_layers, cfg.hidden_dim,
                             cfg.nheads, cfg.dim_feedforward, int(cfg.sigma_head),
                             {"bf16": _lib.SPE_DTYPE_BF16, "fp32": _lib.SPE_DTYPE_F32,
                              "fp32x3": _lib.SPE_DTYPE_F32X3, "fp32x6": _lib.SPE_DTYPE_F32X6,
                              "fp32h3": _lib.SPE_DTYPE_F32H3}[dtype],
                             _lib.SPE_DTYPE_F16 if self.attn_dtype == "fp16" else 0)
        h = ctypes.c_void_p()
        bb = {"resnet50s8": _lib.SPE_BACKBONE_RESNET50_S8, "resnet50": _lib.SPE_BACKBONE_RESNET50_S16}[cfg.backbone]
        flags = (_lib.SPE_MODEL_PRE_NORM if cfg.pre_norm else 0) | \
                (_lib.SPE_MODEL_GROUP_NORM if cfg.norm == "group_bn" else 0)
        _lib.check(L.spe_model_create_flags(ctypes.byref(c), bb, flags, ctypes.byref(h)), "spe_model_create_flags")
        self._adopt(h)

    # ---------------------------------------------------------------- forward
    def _outputs(self, B, dev, clip_bbox, return_hs):
        Q = self.cfg.num_queries
        out = {"pred_logits": torch.empty(B, Q, 12, device=dev), "pred_points": torch.empty(B, Q, 2, device=dev)}
        if self.cfg.sigma_head:
            out["pred_sigmas"] = torch.empty(B, Q, 2, device=dev)
            out["sigmas"] = torch.empty(B, Q, 2, device=dev)
        if return_hs:
            out["hs"] = torch.empty(B, Q, self.cfg.hidden_dim, device=dev)
        if clip_bbox is not None:
            out["probs"] = torch.empty(B, Q, 12, device=dev)
            out["points_px"] = torch.empty(B, Q, 2, device=dev)
        aux_l = aux_p = None
        if self.aux_loss and self.cfg.dec_layers > 1:       # REV/models/detr_speed.py:88-99
            aux_l = torch.empty(self.cfg.dec_layers - 1, B, Q, 12, device=dev)
            aux_p = torch.empty(self.cfg.dec_layers - 1, B, Q, 2, device=dev)
            out["aux_outputs"] = [{"pred_logits": a, "pred_points": p} for a, p in zip(aux_l, aux_p)]
        o = _lib.ForwardOutputs(_lib.ptr(out["pred_logits"]), _lib.ptr(out["pred_points"]), _lib.ptr(clip_bbox),
                                _lib.ptr(out.get("probs")), _lib.ptr(out.get("points_px")),
                                _lib.ptr(out.get("pred_sigmas")), _lib.ptr(out.get("sigmas")),
                                _lib.ptr(out.get("hs")), _lib.ptr(aux_l), _lib.ptr(aux_p))
        return out, o

    def encode(self, images, ws, stream=None, part=None, B=None):
        """Encode stage (backbone, neck (resnet50s8), input_proj, encoder): images -> memory kept in `ws`.
        part="backbone": up to input_proj (images -> src in `ws`); part="transformer": the
        encoder layers over the src a backbone part left in `ws` (images may be None, B given)."""
        stage = {None: _lib.SPE_STAGE_ENCODE, "backbone": _lib.SPE_STAGE_BACKBONE,
                 "transformer": _lib.SPE_STAGE_TRANSFORMER}[part]
        self._run(images, images.shape[0] if images is not None else int(B), ws, stream, None, stage)

    def decode(self, B, ws, clip_bbox=None, stream=None, return_hs=False):
        """Decode stage (decoder, heads, fused PostProcess) of the memory an encode() left in `ws`."""
        out, o = self._outputs(B, ws.device, self._clip(clip_bbox, ws.device), return_hs)
        self._run(None, B, ws, stream, o, _lib.SPE_STAGE_DECODE)
        return out

    def forward(self, samples, clip_bbox=None, stream=None, return_hs=False):
        """REV/models/detr_speed.py:59-92.  Returns pred_logits [B,Q,12], pred_points [B,Q,2]
        (+ pred_sigmas as log-sigma when the sigma head is configured).  Passing `clip_bbox`
        ([B,4] device fp32) also runs the fused PostProcess and adds `probs` / `points_px`."""
        self._require_ready("forward")
        images = self._unwrap(samples)
        if images.is_cuda and images.dtype == torch.uint8:
            self._crop_channels(images)       # the 8-bit crops to_tensor + Normalize would make the batch from
        else:
            images = self._fp32_batch(images)
        B, dev = images.shape[0], images.device
        out, o = self._outputs(B, dev, self._clip(clip_bbox, dev), return_hs)
        self._run(images, B, self.workspace(B, dev, stream), stream, o, _lib.SPE_STAGE_ENCODE | _lib.SPE_STAGE_DECODE)
        return out

    def forward_with_attention(self, images, enc_layer=-1, dec_layer=-2, clip_bbox=None, *, stream=None, maps=None):
        """forward() plus the attention maps the reference's visualize_features.py hooks: the head-averaged
        probabilities of transformer.encoder.layers[enc_layer].self_attn ("enc", [B,T,T], T = cfg.tokens:
        (S/8)^2, or (S/16)^2 with the plain resnet50 backbone) and transformer.decoder.layers[dec_layer].multihead_attn ("dec", [B,Q,T]), device fp32.
        Returns (outputs, maps); `outputs` is forward()'s dict, bit for bit.  Model dtypes bf16 and fp32.
        `maps` (optional): {"enc": tensor or None, "dec": tensor or None} of caller buffers to fill; None
        skips that tap (spe_forward_attention's NULL map)."""
        self._require_ready("forward_with_attention")
        images = self._fp32_batch(images)
        B, dev = images.shape[0], images.device
        out, o = self._outputs(B, dev, self._clip(clip_bbox, dev), False)
        T = self.cfg.tokens
        shapes = {"enc": (B, T, T), "dec": (B, self.cfg.num_queries, T)}
        if maps is None:
            maps = {k: torch.empty(*s, device=dev) for k, s in shapes.items()}
        else:
            maps = {k: maps.get(k) for k in shapes}
            for k, t in maps.items():
                if t is not None and (tuple(t.shape) != shapes[k] or t.dtype != torch.float32 or t.device != dev
                                      or not t.is_contiguous()):
                    raise ValueError(f"maps[{k!r}]: a contiguous fp32 {shapes[k]} tensor on {dev}")
        L = _lib.lib()
        ws = self.workspace(B, dev, stream)
        if ws.numel() < int(L.spe_forward_attention_workspace_bytes(self._h, B)):
            raise RuntimeError("forward_with_attention: the forward workspace no longer covers the taps")
        _lib.check(L.spe_forward_attention(self._h, _lib.stream_ptr(stream), _lib.ptr(images), B, _lib.ptr(ws),
                                           ws.numel(), ctypes.byref(o), int(enc_layer), int(dec_layer),
                                           _lib.ptr(maps["enc"]), _lib.ptr(maps["dec"])), "spe_forward_attention")
        return out, {k: t for k, t in maps.items() if t is not None}


class SetCriterion(nn.Module):
    """REV/models/detr_speed.py:103-261 with the HungarianMatcher of REV/models/matcher.py:35-88,
    on the device (spe_criterion, csrc/criterion.hip): one launch matches and scores the last
    layer and every aux layer.  Returns the reference's loss dict (loss_ce, class_error,
    loss_points, cardinality_error, and *_i for aux layer i without class_error) as 0-d device
    tensors; `weight_dict` as REV/models/detr_speed.py:319-327 builds it.  The matching of the
    last call is kept in `last_match` ([L,B,T] query per target; layer L-1 = last)."""

    def __init__(self, num_classes: int = 11, cost_class: float = 1.0, cost_pts: float = 5.0,
                 eos_coef: float = 0.1, pts_loss_coef: float = 5.0, dec_layers: int = 6, aux_loss: bool = True):
        super().__init__()
        self.num_classes, self.cost_class, self.cost_pts, self.eos_coef = num_classes, cost_class, cost_pts, eos_coef
        self.weight_dict = {"loss_ce": 1, "loss_points": pts_loss_coef}
        if aux_loss:
            for i in range(dec_layers - 1):
                self.weight_dict.update({f"loss_ce_{i}": 1, f"loss_points_{i}": pts_loss_coef})
        self.last_match = None

    @torch.no_grad()
    def forward(self, outputs, targets, stream=None):
        layers = [(a["pred_logits"], a["pred_points"]) for a in outputs.get("aux_outputs", [])]
        layers.append((outputs["pred_logits"], outputs["pred_points"]))
        logits = torch.stack([l for l, _ in layers]).float().contiguous()
        points = torch.stack([p for _, p in layers]).float().contiguous()
        L, B, Q, C = logits.shape
        dev = logits.device
        labels = torch.stack([t["labels"] for t in targets]).to(dev, torch.int32).contiguous()
        tpts = torch.stack([t["landmarks"] for t in targets]).to(dev, torch.float32).contiguous()
        T = labels.shape[1]
        num_points = float(B * T)                         # REV/models/detr_speed.py:235-244
        from . import dist as spe_dist
        if spe_dist.is_dist():
            n = torch.tensor([num_points], dtype=torch.float64, device=dev)
            torch.distributed.all_reduce(n)
            num_points = float(n.item()) / torch.distributed.get_world_size()
        num_points = max(num_points, 1.0)
        match = torch.empty(L, B, T, dtype=torch.int32, device=dev)
        res = torch.empty(L, 4, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().spe_criterion(_lib.stream_ptr(stream), _lib.ptr(logits), _lib.ptr(points), _lib.ptr(labels),
                                            _lib.ptr(tpts), L, B, Q, C, T, self.cost_class, self.cost_pts,
                                            self.eos_coef, num_points, _lib.ptr(match), _lib.ptr(res)), "spe_criterion")
        self.last_match = match
        losses = {}
        for l in range(L):
            sfx = "" if l == L - 1 else f"_{l}"
            losses["loss_ce" + sfx] = res[l, 0]
            if l == L - 1:
                losses["class_error"] = res[l, 1]
            losses["cardinality_error" + sfx] = res[l, 2]
            losses["loss_points" + sfx] = res[l, 3]
        return losses


class PostProcess(nn.Module):
    """REV/models/detr_speed.py:264-293 (and the sigma variant,
    UNC/src/zoo/rtdetr/rtdetr_postprocessor.py:44-78): softmax over the 12 classes and
    crop -> image pixel rescale, on device; returns the reference's list of numpy dicts."""

    @torch.no_grad()
    def forward(self, outputs, clip_bbox, stream=None):
        logits, points = outputs["pred_logits"], outputs["pred_points"]
        B, Q, _ = logits.shape
        assert len(clip_bbox) == B
        dev = logits.device
        bb = torch.stack([torch.as_tensor(b, dtype=torch.float32) for b in clip_bbox]).to(dev)
        if "probs" in outputs and "points_px" in outputs:
            probs, pts = outputs["probs"], outputs["points_px"]
        else:
            probs = torch.empty_like(logits)
            pts = torch.empty_like(points)
            _lib.check(_lib.lib().spe_postprocess(_lib.stream_ptr(stream), _lib.ptr(logits.contiguous()),
                                                   _lib.ptr(points.contiguous()), _lib.ptr(bb), B, Q,
                                                   _lib.ptr(probs), _lib.ptr(pts)), "spe_postprocess")
        probs, pts = probs.cpu().numpy(), pts.cpu().numpy()
        res = [{"logits": probs[i], "points": pts[i]} for i in range(B)]
        if "sigmas" in outputs:
            sg = outputs["sigmas"].cpu().numpy()
            for i in range(B):
                res[i]["sigmas"] = sg[i]
        return res


def build_model(args, dtype: str = None):
    """REV/models/__init__.py:5-6 / detr_speed.py:296-336.  Returns (model, criterion,
    postprocessors); the criterion is the device SetCriterion with the reference's argparse
    defaults (set_cost_class 1, set_cost_pts 5, eos_coef 0.1, pts_loss_coef 5)."""
    cfg = SpeConfig.from_args(args)
    dtype = dtype or getattr(args, "dtype", "bf16")
    aux = bool(getattr(args, "aux_loss", False))
    model = DETR(cfg, dtype=dtype, aux_loss=aux, attn_dtype=getattr(args, "attn_dtype", None))
    criterion = SetCriterion(cost_class=float(getattr(args, "set_cost_class", 1.0)),
                             cost_pts=float(getattr(args, "set_cost_pts", 5.0)),
                             eos_coef=float(getattr(args, "eos_coef", 0.1)),
                             pts_loss_coef=float(getattr(args, "pts_loss_coef", 5.0)),
                             dec_layers=cfg.dec_layers, aux_loss=aux)
    return model, criterion, {"points": PostProcess()}
