"""CPU: the attention-map restatements (tests/attention_map_ref.py), the heat-map helpers
(spe/attention_maps.py) and the argument checks of spe_forward_attention, none of which touches a device."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import attention_map_ref as R
import model_ref
from spe import _lib
from spe.attention_maps import decoder_heatmaps, encoder_heatmaps_at
from spe.config import SpeConfig
from spe.synthetic import random_weights, synthetic_batch


def test_restatement_rows_sum_to_one():
    q, k = R.kernel_case(11, 65, seed=3)
    p = R.head_avg_probs(q.double(), k.double())
    assert p.shape == (2, 11, 65)
    assert (p >= 0).all() and (p.sum(-1) - 1).abs().max() < 1e-12
    g = torch.Generator().manual_seed(4)
    qf, kf = torch.randn(2, 5, 8 * 256, generator=g).double() * 0.5, torch.randn(2, 33, 256, generator=g).double() * 0.5
    pf = R.head_avg_probs_folded(qf, kf)
    assert pf.shape == (2, 5, 33) and (pf.sum(-1) - 1).abs().max() < 1e-12


def test_restatement_equals_torch_multi_head_attention():
    """mha_weights_from_inputs against torch's own need_weights=True output (head-averaged)."""
    torch.manual_seed(0)
    d, H, B, Lq, Lk = 256, 8, 2, 7, 19
    W, b = torch.randn(3 * d, d, dtype=torch.float64) * 0.08, torch.randn(3 * d, dtype=torch.float64) * 0.1
    Wo, bo = torch.randn(d, d, dtype=torch.float64) * 0.05, torch.zeros(d, dtype=torch.float64)
    q_in, k_in = torch.randn(B, Lq, d, dtype=torch.float64), torch.randn(B, Lk, d, dtype=torch.float64)
    _, w = F.multi_head_attention_forward(q_in.transpose(0, 1), k_in.transpose(0, 1), k_in.transpose(0, 1), d, H, W, b,
                                          None, None, False, 0.0, Wo, bo, training=False, need_weights=True)
    sd = {"a.in_proj_weight": W, "a.in_proj_bias": b}
    mine = R.mha_weights_from_inputs(q_in, k_in, sd, "a", H)
    assert w.shape == mine.shape == (B, Lq, Lk)
    assert (w - mine).abs().max() < 1e-14


def test_folded_form_equals_the_plain_one():
    """The bf16 decoder's fold (registry.cpp fold_cross_attention): q' = s Wk_h^T q_h against the raw key input
    gives the softmax of q_h . k_h (the key bias drops out)."""
    torch.manual_seed(1)
    d, H, hd, B, Lq, Lk = 256, 8, 32, 1, 3, 9
    Wq, Wk = torch.randn(d, d, dtype=torch.float64) * 0.1, torch.randn(d, d, dtype=torch.float64) * 0.1
    bq, bk = torch.randn(d, dtype=torch.float64), torch.randn(d, dtype=torch.float64)
    x, mem = torch.randn(B, Lq, d, dtype=torch.float64), torch.randn(B, Lk, d, dtype=torch.float64)
    q = F.linear(x, Wq, bq).view(B, Lq, H, hd).transpose(1, 2)
    k = F.linear(mem, Wk, bk).view(B, Lk, H, hd).transpose(1, 2)
    s = hd ** -0.5 * 1.4426950408889634
    qf = torch.stack([s * q[:, h] @ Wk[h * hd:(h + 1) * hd] for h in range(H)], dim=2).reshape(B, Lq, H * d)
    assert (R.head_avg_probs_folded(qf, mem) - R.head_avg_probs(q, k)).abs().max() < 1e-13


def test_oracle_capture_runs_the_oracle_model():
    """oracle_attention_maps in float32 is model_ref.forward (same functions, same order): equal outputs."""
    cfg = SpeConfig(input_size=64, enc_layers=1, dec_layers=2)
    w, b = random_weights(cfg, 3), synthetic_batch(cfg, 1, 5)
    with torch.no_grad():
        ref = model_ref.forward(b["images"], w, cfg)
        out, enc, dec = R.oracle_attention_maps(b["images"], w, cfg)
    assert torch.equal(out["pred_points"], ref["pred_points"]) and torch.equal(out["pred_logits"], ref["pred_logits"])
    assert len(enc) == 1 and enc[0].shape == (1, 64, 64) and len(dec) == 2 and dec[0].shape == (1, cfg.num_queries, 64)
    assert (enc[0].sum(-1) - 1).abs().max() < 1e-5 and (dec[1].sum(-1) - 1).abs().max() < 1e-5


def test_decoder_heatmaps_one_hot():
    feat, B, Q = 5, 2, 3
    m = torch.zeros(B, Q, feat * feat)
    m[1, 2, 3 * feat + 4] = 1.0                      # image 1, query 2 looks at token (y 3, x 4)
    h = decoder_heatmaps(m, feat)
    assert h.shape == (B, Q, feat, feat)
    assert h[1, 2, 3, 4] == 1.0 and h.sum() == 1.0
    assert decoder_heatmaps(m.numpy(), feat).shape == (B, Q, feat, feat)


def test_encoder_heatmaps_pick_the_token_under_the_keypoint():
    """The reference shows weight.reshape(f, f, f, f)[..., int(py), int(px)]: the weight every (query) token
    puts on the (key) token under the keypoint."""
    feat, B = 4, 1
    T = feat * feat
    m = torch.zeros(B, T, T)
    m[0, 2 * feat + 1, 3 * feat + 0] = 1.0           # query token (y 2, x 1) looks only at key token (y 3, x 0)
    pts = torch.tensor([[[0.10, 0.80],               # (x, y) -> cell x 0, y 3: the key above
                         [0.60, 0.30],               # cell x 2, y 1: nobody looks there
                         [1.00, 1.00]]])             # a saturated sigmoid: clamped to the last cell
    h = encoder_heatmaps_at(m, pts, feat)
    assert h.shape == (B, 3, feat, feat)
    assert h[0, 0, 2, 1] == 1.0 and h[0, 0].sum() == 1.0
    assert h[0, 1].sum() == 0.0 and h[0, 2].sum() == 0.0
    want = m.reshape(feat, feat, feat, feat).numpy()[..., int(0.80 * feat), int(0.10 * feat)]
    np.testing.assert_array_equal(h[0, 0].numpy(), want)


def _detr(cfg, dtype):
    L = _lib.lib()
    c = _lib.ModelConfig(cfg.input_size, cfg.num_queries, cfg.enc_layers, cfg.dec_layers, cfg.hidden_dim, cfg.nheads,
                         cfg.dim_feedforward, int(cfg.sigma_head), dtype)
    h = ctypes.c_void_p()
    assert L.spe_model_create(ctypes.byref(c), ctypes.byref(h)) == 0
    return h


def test_forward_attention_refusals_come_before_the_device():
    """SPE_E_ARG (-1) for an RT-DETR handle, the split-precision modes, both maps NULL and a layer index out
    of range; every pointer below is a dummy that is never dereferenced."""
    from spe.rtdetr_spec import RtdetrConfig
    L = _lib.lib()
    dummy = ctypes.c_void_p(16)
    out = _lib.ForwardOutputs(dummy, dummy, None, None, None, None, None, None, None, None)

    def call(h, el, dl, em, dm):
        return L.spe_forward_attention(h, None, dummy, 1, dummy, 1 << 40, ctypes.byref(out), el, dl, em, dm)

    r = RtdetrConfig(depth=18, input_size=128)
    c = _lib.RtdetrConfig(r.depth, r.input_size, r.num_queries, r.dec_layers, r.enc_ff, r.dec_ff, r.csp_hidden,
                          r.num_classes, _lib.SPE_DTYPE_BF16)
    h = ctypes.c_void_p()
    assert L.spe_rtdetr_create(ctypes.byref(c), ctypes.byref(h)) == 0
    assert call(h, -1, -2, dummy, dummy) == -1 and b"not a DETR model" in L.spe_last_error()
    L.spe_model_destroy(h)

    cfg = SpeConfig(input_size=128, enc_layers=2, dec_layers=2)
    for dt in (_lib.SPE_DTYPE_F32X3, _lib.SPE_DTYPE_F32X6, _lib.SPE_DTYPE_F32H3):
        h = _detr(cfg, dt)
        assert call(h, -1, -2, dummy, dummy) == -1
        msg = L.spe_last_error()
        assert b"bf16" in msg and b"fp32" in msg, msg      # names the supported modes
        L.spe_model_destroy(h)

    for dt in (_lib.SPE_DTYPE_BF16, _lib.SPE_DTYPE_F32):
        h = _detr(cfg, dt)
        assert call(h, -1, -2, None, None) == -1 and b"both null" in L.spe_last_error()
        for el, dl, em, dm in ((2, -2, dummy, dummy), (-3, -2, dummy, dummy), (-1, 2, dummy, dummy),
                               (-1, -3, dummy, dummy), (-1, 5, None, dummy), (7, 0, dummy, None)):
            assert call(h, el, dl, em, dm) == -1 and b"out of range" in L.spe_last_error(), (el, dl)
        # an index that is out of range for a skipped tap is not looked at: the call then reaches the model
        # checks (not finalized, SPE_E_STATE), still before any launch
        assert call(h, 9, 0, None, dummy) == -2
        assert L.spe_forward_attention_workspace_bytes(h, 2) == L.spe_model_workspace_bytes(h, 2) > 0
        L.spe_model_destroy(h)
    assert L.spe_debug_attn_map(None, dummy, dummy, 1, 4, 8, 8, _lib.SPE_DTYPE_F32, dummy) == -1     # H != 8
    assert L.spe_debug_attn_map(None, dummy, dummy, 1, 8, 8, 8, 7, dummy) == -1                      # no such dtype
