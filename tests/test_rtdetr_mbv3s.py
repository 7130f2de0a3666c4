"""UNC RT-DETR behind the MobileNetV3_Small backbone (UNC/nn/backbone/mobilenetv3.py:228-320), CPU side: the
parameter space equals the reference model's own state_dict (tests/golden/rtdetr_keys_mbv3s.json), the torch-fp32
restatement (tests/rtdetr_mbv3s_ref.py) reproduces the reference's outputs recorded by
tools/gen_golden_rtdetr_mbv3s.py, the fp64 reference of the fused entry kernel composes to the restatement's
block-0 inputs, and the C ABI builds the handle at 256, refuses every other size and leaves the other light
backbones' key spaces alone.

Tolerances are tests/test_rtdetr_mbv3.py's: restatement vs reference pred_pts / pred_sigmas |d| <= 1e-5, logits
|d| <= 1e-4, backbone map samples 1e-5, top-k exact.  Exact top-k is a fair demand on this golden: its
topk_min_gap is 1.439e-3, the largest encoder-score difference between the restatement and the reference
measured when the golden was written is 4.053e-6 (both stored in the golden; the seeds were chosen for gap >=
10 x difference).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from spe.config import SpeConfig
from spe.rtdetr_spec import (MBV3_SMALL_BLOCKS, RtdetrConfig, mbv3_small_param_shapes, random_rtdetr_weights,
                             rtdetr_param_shapes)
from spe.synthetic import synthetic_batch
import rtdetr_mbv3s_ref as R
from rtdetr_mbv3_ref import se_module

MB = dict(backbone="MobileNetV3_Small")


def golden():
    g = np.load(os.path.join(GOLDEN, "rtdetr_mbv3s_s256.npz"))
    cfg = RtdetrConfig(**json.loads(str(g["config"])))
    return g, cfg


def _chk(a):
    a = np.asarray(a, np.float64)
    return np.array([a.sum(), np.abs(a).sum(), (a * a).sum(), a.ravel()[:: max(1, a.size // 97)].sum()])


_ref = {}


def reference_run():
    """The restatement on the golden's weights and images, computed once and shared (read-only)."""
    if not _ref:
        g, cfg = golden()
        w = random_rtdetr_weights(cfg, int(g["weight_seed"]))
        b = synthetic_batch(SpeConfig(input_size=cfg.input_size), int(g["batch"]), int(g["image_seed"]))
        trace = {}
        o = R.forward(b["images"], w, cfg, trace)
        _ref.update(g=g, cfg=cfg, w=w, batch=b, trace=trace, out=o)
    return _ref


def _ref_keys(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return [(k, tuple(s)) for k, s in json.load(f) if not k.endswith("num_batches_tracked")]


def test_param_space_matches_reference_state_dict():
    ref = _ref_keys("rtdetr_keys_mbv3s.json")
    bb = [(k, s) for k, s in ref if k.startswith("backbone.")]
    assert [k for k, _ in bb[:4]] == ["backbone.conv1.weight", "backbone.Conv1.weight", "backbone.Conv2.weight",
                                      "backbone.bn1.weight"]
    cfg = RtdetrConfig(**MB)
    mine = [(k, tuple(s)) for k, s in rtdetr_param_shapes(cfg)]
    assert mine == ref
    assert [(k, tuple(s)) for k, s in mbv3_small_param_shapes()] == bb
    keys = [k for k, _ in mine]
    assert "backbone.linear3.weight" in keys and "backbone.bn3.running_var" in keys and "backbone.Bn1.weight" not in keys
    assert "backbone.bneck.0.skip.1.weight" in keys and "backbone.bneck.0.skip.2.weight" not in keys
    assert len(MBV3_SMALL_BLOCKS) == 11 and cfg.backbone_channels == [128, 256, 512]


def test_restatement_matches_reference_golden():
    r = reference_run()
    g, trace, o = r["g"], r["trace"], r["out"]
    np.testing.assert_allclose(_chk(r["batch"]["images"]), g["input_checksum"], rtol=1e-6)
    stride = int(g["sample_stride"])
    for i, t in enumerate(trace["feats"]):
        np.testing.assert_allclose(_chk(t.numpy()), g[f"chk_feat{i}"], rtol=1e-4)
        np.testing.assert_allclose(t.numpy().ravel()[::stride], g[f"feat{i}_sample"], atol=1e-5)
    for i, t in enumerate(trace["enc"]):
        np.testing.assert_allclose(_chk(t.numpy()), g[f"chk_enc{i}"], rtol=1e-4)
    assert float(g["topk_min_gap"]) >= 10 * float(g["oracle_score_diff"])
    np.testing.assert_array_equal(trace["topk"].numpy(), g["topk_ind"])
    np.testing.assert_allclose(o["pred_pts"].numpy(), g["pred_pts"], atol=1e-5)
    np.testing.assert_allclose(o["pred_sigmas"].numpy(), g["pred_sigmas"], atol=1e-5)
    np.testing.assert_allclose(o["pred_logits"].numpy(), g["pred_logits"], atol=1e-4)
    np.testing.assert_allclose(o["aux_pts"].numpy(), g["aux_pts"], atol=1e-5)
    np.testing.assert_allclose(o["aux_sigmas"].numpy(), g["aux_sigmas"], atol=1e-5)
    np.testing.assert_allclose(o["aux_logits"].numpy(), g["aux_logits"], atol=1e-4)
    np.testing.assert_allclose(o["enc_topk_logits"].numpy(), g["enc_topk_logits"], atol=1e-4)
    np.testing.assert_allclose(o["enc_topk_bboxes"].numpy(), g["enc_topk_bboxes"], atol=1e-5)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_folded_restatement_equals_the_definition(fused):
    """The forms the HIP model computes (BatchNorm folded, the 64 x 64 resize as an exact 2 x 2 mean, block 0
    through the entry's three maps or launch by launch) are the same function: identity rounder, fp32 rounding
    differences only (the Large test's 1e-4)."""
    r = reference_run()
    x = torch.from_numpy(r["batch"]["images"])
    with torch.no_grad():
        folded = R.mobilenetv3_small_rounded(x, r["w"], lambda t: t, fused=fused)
    for a, b in zip(folded, r["trace"]["feats"]):
        assert (a - b).abs().max().item() <= 1e-4


def test_entry_reference_composes_to_block0_inputs():
    """entry_ref64 on the golden's weights: its stem is the restatement's stem map, its pooled map is the
    bilinear 64 x 64 resize, and skip / t2 are what Block 0 computes from the stem map -- pushing them through
    the rest of block 0 (SE gate, project, residual, ReLU) gives the restatement's block-0 output.  fp64 against
    fp32 torch: 2e-5 on values up to ~8."""
    r = reference_run()
    w, trace = r["w"], r["trace"]
    x = torch.from_numpy(r["batch"]["images"])
    e = R.entry_ref64(x, R.entry_weights(w))
    nchw = lambda t: t.permute(0, 3, 1, 2)
    assert (nchw(e["stem"]) - trace["stem"]).abs().max().item() <= 2e-5
    resized = F.interpolate(trace["stem"], size=(64, 64), mode="bilinear", align_corners=False)
    assert (nchw(e["pooled"]) - resized).abs().max().item() <= 2e-5
    p = "backbone.bneck.0"
    t2 = nchw(e["t2"]).float()
    with torch.no_grad():
        o = se_module(t2, w, f"{p}.se")
        o = R._bn(F.conv2d(o, R._t(w, f"{p}.conv3.weight")), w, f"{p}.bn3")
        out0 = F.relu(o + nchw(e["skip"]).float())
    assert (out0 - trace["block_out"][0]).abs().max().item() <= 2e-5
    # the padding the kernel must reproduce: zero outside the stem map, not act(bias)
    wb = R.entry_random_weights(3)
    xs = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(0))
    a = R.entry_ref64(xs, wb)
    assert a["stem"].shape == (1, 16, 16, 16) and a["t2"].shape == (1, 8, 8, 16)
    b16 = wb[R.W_STEM_B:R.W_STEM_B + 16].double()
    assert (b16 * F.relu6(b16 + 3.0) / 6.0).abs().min().item() > 0.05


def test_crop_normalisation_order():
    u = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16)
    x = R.normalise_crops(u)
    assert x.shape == (1, 3, 16, 16) and x.dtype == torch.float32
    want = (np.float32(200) / np.float32(255) - np.float32(0.456)) / np.float32(0.224)
    assert x[0, 1, 12, 8].item() == want.item()


def _create(selector, size):
    from spe import _lib
    c = _lib.RtdetrConfig(selector, size, 30, 3, 1024, 1024, 128, 11, _lib.SPE_DTYPE_F32)
    h = ctypes.c_void_p()
    return _lib.lib().spe_rtdetr_create(ctypes.byref(c), ctypes.byref(h)), h


def _handle_keys(selector):
    from spe import _lib
    L = _lib.lib()
    rc, h = _create(selector, 256)
    assert rc == 0 and h.value, L.spe_last_error()
    try:
        return [L.spe_model_param_name(h, i).decode() for i in range(L.spe_model_num_params(h))]
    finally:
        L.spe_model_destroy(h)


def test_capi_create_accepts_256_and_lists_the_reference_keys():
    from spe import _lib
    assert _lib.ABI_VERSION == 9 and _lib.lib().spe_abi_version() == 9 and _lib.SPE_RTDETR_MBV3_SMALL == 1005
    assert _handle_keys(_lib.SPE_RTDETR_MBV3_SMALL) == [k for k, _ in _ref_keys("rtdetr_keys_mbv3s.json")]


@pytest.mark.parametrize("size", [224, 512])
def test_capi_create_refuses_other_sizes(size):
    from spe import _lib
    rc, h = _create(_lib.SPE_RTDETR_MBV3_SMALL, size)
    assert rc == -1 and not h.value
    msg = _lib.lib().spe_last_error().decode()
    assert "64x64" in msg and "256" in msg


def test_capi_other_light_selectors_unchanged():
    from spe import _lib
    assert _handle_keys(_lib.SPE_RTDETR_MBV3_LARGE) == [k for k, _ in _ref_keys("rtdetr_keys_mbv3l.json")]
    assert _handle_keys(_lib.SPE_RTDETR_GHOSTNETV2) == [k for k, _ in _ref_keys("rtdetr_keys_ghostv2.json")]
    rc, h = _create(1006, 256)
    assert rc == -1 and not h.value


def test_model_class_maps_the_backbone_field():
    """RTDETR(cfg) with the new backbone lists the reference's keys; a reference-keyed state_dict
    (num_batches_tracked included) leaves nothing missing or unexpected -- host side only (finalize needs a
    device, so one key is held back)."""
    from spe.rtdetr import RTDETR
    cfg = RtdetrConfig(**MB)
    m = RTDETR(cfg, "fp32")
    with open(os.path.join(GOLDEN, "rtdetr_keys_mbv3s.json")) as f:
        full = [(k, tuple(s)) for k, s in json.load(f)]
    w = random_rtdetr_weights(cfg, 0)
    sd = {k: (w[k] if k in w else np.zeros(s, np.int64)) for k, s in full}
    assert set(w) == {k for k, _ in full if not k.endswith("num_batches_tracked")}
    held = "backbone.bn3.running_var"          # a never-called parameter: still a required key
    sd.pop(held)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert missing == [held] and unexpected == []
    with pytest.raises(Exception):
        RTDETR(RtdetrConfig(input_size=128, **MB), "fp32")
