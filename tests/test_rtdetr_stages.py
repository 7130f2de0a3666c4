"""CPU: the staged RT-DETR entry points (spe_rtdetr_forward_stages / _u8, include/spe.h) are exported,
refuse every malformed call before any launch, and spe.rtdetr.RTDETR carries the staging surface
PosePipeline drives (new_workspace, encode, decode) and the 8-bit crop check of its forward."""
import ctypes
import inspect

import pytest
import torch

from spe import _lib
from spe.config import SpeConfig
from spe.rtdetr_spec import RtdetrConfig

ARG, STATE = -1, -2
B, T, D, E = _lib.SPE_STAGE_BACKBONE, _lib.SPE_STAGE_TRANSFORMER, _lib.SPE_STAGE_DECODE, _lib.SPE_STAGE_ENCODE
DUMMY = ctypes.c_void_p(16)          # never dereferenced: every refusal comes before the first launch


@pytest.fixture()
def r18():
    """An r18 handle at S=128 with no parameter set: not finalized."""
    L = _lib.lib()
    r = RtdetrConfig(depth=18, input_size=128)
    c = _lib.RtdetrConfig(r.depth, r.input_size, r.num_queries, r.dec_layers, r.enc_ff, r.dec_ff, r.csp_hidden,
                          r.num_classes, _lib.SPE_DTYPE_BF16)
    h = ctypes.c_void_p()
    assert L.spe_rtdetr_create(ctypes.byref(c), ctypes.byref(h)) == 0
    yield h
    L.spe_model_destroy(h)


def _out(logits=DUMMY, points=DUMMY):
    return _lib.RtdetrOutputs(logits, points, *([None] * 12))


def _f32(h, stages, images=DUMMY, out=None, batch=1, ws=DUMMY):
    o = ctypes.byref(out) if out is not None else None
    return _lib.lib().spe_rtdetr_forward_stages(h, None, images, batch, ws, 1 << 40, o, stages)


def _u8(h, stages, crops=DUMMY, ch=1, out=None, batch=1, ws=DUMMY):
    o = ctypes.byref(out) if out is not None else None
    return _lib.lib().spe_rtdetr_forward_stages_u8(h, None, crops, ch, batch, ws, 1 << 40, o, stages)


def test_symbols_exported_and_abi_unchanged():
    L = _lib.lib()
    for name in ("spe_rtdetr_forward_stages", "spe_rtdetr_forward_stages_u8"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.spe_abi_version() == _lib.ABI_VERSION == 9


def test_null_arguments_refused(r18):
    L = _lib.lib()
    for call in (_f32, _u8):
        assert call(None, E | D, out=_out()) == ARG
        assert call(r18, E | D, out=_out(), ws=None) == ARG
        assert call(r18, E | D, out=_out(), batch=0) == ARG
        assert call(r18, E | D, out=_out(), batch=-3) == ARG
        assert b"bad argument" in L.spe_last_error()


def test_detr_handle_refused():
    L = _lib.lib()
    cfg = SpeConfig()
    c = _lib.ModelConfig(cfg.input_size, cfg.num_queries, cfg.enc_layers, cfg.dec_layers, cfg.hidden_dim, cfg.nheads,
                         cfg.dim_feedforward, int(cfg.sigma_head), _lib.SPE_DTYPE_BF16)
    h = ctypes.c_void_p()
    assert L.spe_model_create(ctypes.byref(c), ctypes.byref(h)) == 0
    for call in (_f32, _u8):
        assert call(h, E | D, out=_out()) == ARG
        assert b"not an RT-DETR model" in L.spe_last_error()
        assert call(h, 0) == ARG                       # the family check comes before the mask's
        assert b"not an RT-DETR model" in L.spe_last_error()
    L.spe_model_destroy(h)


@pytest.mark.parametrize("stages", [0, 16, 32 | E, -1, B | D, B | D | 64])
def test_bad_stage_masks_refused(r18, stages):
    L = _lib.lib()
    for call in (_f32, _u8):
        assert call(r18, stages, out=_out()) == ARG
        assert b"stages" in L.spe_last_error()


@pytest.mark.parametrize("stages", [B, T, D, E, B | T, T | D, E | D, B | T | D, E | B, E | T | D])
def test_good_stage_masks_reach_the_state_check(r18, stages):
    """Every single stage and every run of neighbours passes the argument checks: the handle is not
    finalized, so the call ends at SPE_E_STATE, still before any launch."""
    L = _lib.lib()
    for call in (_f32, _u8):
        assert call(r18, stages, out=_out()) == STATE
        assert b"not finalized" in L.spe_last_error()


def test_backbone_needs_images_and_decode_needs_outputs(r18):
    L = _lib.lib()
    for call in (_f32, _u8):
        for stages in (B, E, E | D, B | T):
            assert call(r18, stages, None, out=_out()) == ARG
            assert b"null images" in L.spe_last_error()
        for stages in (D, T | D, E | D):
            assert call(r18, stages, out=None) == ARG
            assert call(r18, stages, out=_out(logits=None)) == ARG
            assert call(r18, stages, out=_out(points=None)) == ARG
            assert b"null outputs" in L.spe_last_error()
        # neither is needed by a stage that does not use it
        assert call(r18, T, None, out=None) == STATE
        assert call(r18, D, None, out=_out()) == STATE
        assert call(r18, B, out=None) == STATE


@pytest.mark.parametrize("ch", [0, 2, 4, -1])
def test_u8_channels_refused(r18, ch):
    L = _lib.lib()
    for stages in (B, E | D, D):
        assert _u8(r18, stages, ch=ch, out=_out()) == ARG
        assert b"1 or 3 channels" in L.spe_last_error()
    assert _u8(r18, E | D, ch=3, out=_out()) == STATE


def test_unsplit_entry_still_refuses_in_its_order(r18):
    L = _lib.lib()
    o = _out()
    assert L.spe_rtdetr_forward(r18, None, None, 1, DUMMY, 1 << 40, ctypes.byref(o)) == ARG
    assert L.spe_rtdetr_forward(r18, None, DUMMY, 1, DUMMY, 1 << 40, None) == ARG
    assert L.spe_rtdetr_forward(r18, None, DUMMY, 1, DUMMY, 1 << 40, ctypes.byref(o)) == STATE


def test_rtdetr_has_the_staging_surface_of_detr():
    from spe.models import DETR
    from spe.rtdetr import RTDETR
    for name in ("new_workspace", "encode", "decode", "workspace"):
        assert callable(getattr(RTDETR, name)), name
    for name in ("new_workspace", "encode"):
        assert list(inspect.signature(getattr(RTDETR, name)).parameters) == \
            list(inspect.signature(getattr(DETR, name)).parameters), name
    assert list(inspect.signature(RTDETR.decode).parameters) == ["self", "B", "ws", "clip_bbox", "stream", "aux", "return_hs"]
    m = RTDETR(RtdetrConfig(depth=18, input_size=128))
    with pytest.raises(RuntimeError, match="load_state_dict"):
        m.encode(torch.zeros(1, 3, 128, 128), torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="load_state_dict"):
        m.decode(1, torch.zeros(16, dtype=torch.uint8))


def test_forward_refuses_malformed_u8_crops():
    """DETR._crop_channels' check and text.  The device check comes first, so a host tensor of any shape
    reports the device; the shape check is driven with a stand-in that answers like a device tensor."""
    from spe.rtdetr import RTDETR
    m = RTDETR(RtdetrConfig(depth=18, input_size=128))
    with pytest.raises(ValueError, match="u8 crops: a contiguous device tensor"):
        m(torch.zeros(2, 128, 128, dtype=torch.uint8))
    with pytest.raises(ValueError, match="u8 crops: a contiguous device tensor"):
        m(torch.zeros(2, 64, 64, 3, dtype=torch.uint8))

    class OnDevice:                       # a stand-in with a device tensor's answers and a shape
        is_cuda = True

        def __init__(self, *shape, contiguous=True):
            self.shape, self._c = torch.Size(shape), contiguous

        def is_contiguous(self):
            return self._c

        def dim(self):
            return len(self.shape)

    assert m._crop_channels(OnDevice(2, 128, 128)) == 1
    assert m._crop_channels(OnDevice(5, 128, 128, 3)) == 3
    with pytest.raises(ValueError, match="u8 crops: a contiguous device tensor"):
        m._crop_channels(OnDevice(2, 128, 128, contiguous=False))
    for shape in ((2, 128, 64), (2, 3, 128, 128), (2, 128, 128, 1), (2, 256, 256), (128, 128)):
        with pytest.raises(ValueError, match=r"u8 crops: expected \[B,128,128\] or \[B,128,128,3\], got"):
            m._crop_channels(OnDevice(*shape))
    # every other input behaves as before: a model without its parameters refuses to run
    with pytest.raises(RuntimeError, match="load_state_dict"):
        m(torch.zeros(2, 3, 128, 128))


def test_generate_submission_refuses_the_per_area_solver():
    from spe.engine import generate_submission
    from spe.solver import EPnPCeresSolver
    with pytest.raises(ValueError, match="EPnPCeresSolver"):
        generate_submission(lambda *a, **k: None, None, {"a.jpg": [[0, 0, 1, 1, 1]]}, lambda f: b"", EPnPCeresSolver(256),
                            torch.device("cpu"), 2, 256)
