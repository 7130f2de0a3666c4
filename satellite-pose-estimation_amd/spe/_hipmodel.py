"""What DETR (spe.models) and RTDETR (spe.rtdetr) share over a libspe.so model handle: the parameters, the
workspaces, the input forms and the staged launch.  A subclass creates its handle (_adopt), builds its output
struct (_outputs) and names its entry points; everything else that both do is here, once.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
from torch import nn

from . import _lib
from .misc import NestedTensor, nested_tensor_from_tensor_list


class HipModel(nn.Module):
    _NAME = None          # the class's name in its error texts
    _HOST_INPUT = None    # its refusal of a host tensor
    _STAGES = None        # its staged forward in the C ABI; the 8-bit crop entry is <_STAGES>_u8

    def _adopt(self, h):
        """Takes the handle a create call filled (kept as `_h`) and reads its parameter names."""
        L = _lib.lib()
        self._h = h
        self._keys = [L.spe_model_param_name(h, i).decode() for i in range(L.spe_model_num_params(h))]
        self._pending = {}
        self._ready = False
        self._ws = {}          # (device, stream) -> (workspace, batch it was sized for)

    # ---------------------------------------------------------------- parameters
    def param_keys(self):
        return list(self._keys)

    def load_state_dict(self, state_dict, strict: bool = True):
        """Accepts the reference's state_dict (torch tensors or numpy arrays); BatchNorm num_batches_tracked
        buffers are ignored (FrozenBatchNorm2d drops them, backbone.py:36-42).  Keys outside the inference path
        are reported as unexpected.  Returns (missing, unexpected) like nn.Module; once every parameter is
        there the model is finalized."""
        L = _lib.lib()
        unexpected = []
        for k, v in state_dict.items():
            if k.endswith("num_batches_tracked"):
                continue
            if k not in self._keys:
                unexpected.append(k)
                continue
            a = np.ascontiguousarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32)
            _lib.check(L.spe_model_set_param(self._h, k.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size),
                       f"set_param({k})")
            self._pending[k] = True
        missing = [k for k in self._keys if k not in self._pending]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing={missing[:5]}... unexpected={unexpected[:5]}...")
        if not self._ready and len(self._pending) == len(self._keys):
            _lib.check(L.spe_model_finalize(self._h), "spe_model_finalize")
            self._ready = True
        return missing, unexpected

    def _require_ready(self, what):
        if not self._ready:
            raise RuntimeError(f"{self._NAME}: load_state_dict() with every parameter before {what}()")

    # ---------------------------------------------------------------- workspaces
    def workspace(self, B, device, stream=None):
        """The default workspace of forward() on `stream` (the current stream if None): one per
        (device, stream), so forwards issued on different streams never share intermediates;
        forwards on one stream are ordered by it.  Allocated from torch's caching allocator on
        that stream, so a regrown workspace's old block is only reused in stream order."""
        device = torch.device(device)
        s = stream if stream is not None else torch.cuda.current_stream(device)
        key = (device.index if device.index is not None else torch.cuda.current_device(), s.cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws[1] < B:
            nbytes = _lib.lib().spe_model_workspace_bytes(self._h, B)
            with torch.cuda.stream(s):
                self._ws[key] = ws = (torch.empty(int(nbytes), dtype=torch.uint8, device=device), B)
        return ws[0]

    def new_workspace(self, B, device):
        """A separate workspace for another in-flight batch (encode/decode overlap)."""
        return torch.empty(int(_lib.lib().spe_model_workspace_bytes(self._h, B)), dtype=torch.uint8, device=device)

    # ---------------------------------------------------------------- inputs
    @staticmethod
    def _unwrap(samples):
        """NestedTensor | list[Tensor] | Tensor -> the batch tensor (REV/models/detr_speed.py:74-75)."""
        if isinstance(samples, (list, tuple)):
            samples = nested_tensor_from_tensor_list(list(samples))
        return samples.tensors if isinstance(samples, NestedTensor) else samples

    def _fp32_batch(self, images):
        """A device batch -> contiguous fp32 [B,3,S,S], or the refusal."""
        if not images.is_cuda:
            raise RuntimeError(self._HOST_INPUT)
        images = images.contiguous().float()
        B, C, H, W = images.shape
        S = self.cfg.input_size
        if C != 3 or H != S or W != S:
            raise ValueError(f"expected [B,3,{S},{S}] input, got {tuple(images.shape)}")
        return images

    def _crop_channels(self, crops):
        """8-bit crops [B,S,S] (grayscale) or [B,S,S,3] (RGB), contiguous on the device -> channels."""
        S = self.cfg.input_size
        if not crops.is_cuda or not crops.is_contiguous():
            raise ValueError("u8 crops: a contiguous device tensor")
        if crops.dim() == 3 and tuple(crops.shape[1:]) == (S, S):
            return 1
        if crops.dim() == 4 and tuple(crops.shape[1:]) == (S, S, 3):
            return 3
        raise ValueError(f"u8 crops: expected [B,{S},{S}] or [B,{S},{S},3], got {tuple(crops.shape)}")

    @staticmethod
    def _clip(clip_bbox, dev):
        """clip_bbox as the fused post-process reads it: fp32, contiguous, on `dev`; None stays None."""
        return clip_bbox.to(device=dev, dtype=torch.float32).contiguous() if clip_bbox is not None else None

    # ---------------------------------------------------------------- launch
    def _run(self, images, B, ws, stream, o, stages):
        """The stages of one forward over `ws`: fp32 images, 8-bit crops, or None without a backbone stage."""
        L = _lib.lib()
        out = ctypes.byref(o) if o is not None else None
        if images is not None and images.dtype == torch.uint8:
            ch = self._crop_channels(images)
            _lib.check(getattr(L, self._STAGES + "_u8")(self._h, _lib.stream_ptr(stream), _lib.ptr(images), ch, B,
                                                        _lib.ptr(ws), ws.numel(), out, stages), self._STAGES + "_u8")
            return
        _lib.check(getattr(L, self._STAGES)(self._h, _lib.stream_ptr(stream), _lib.ptr(images), B, _lib.ptr(ws),
                                            ws.numel(), out, stages), self._STAGES)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().spe_model_destroy(self._h)
                self._h = None
        except Exception:
            pass
