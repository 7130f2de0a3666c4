"""CPU: the RT-DETR attention-map restatement (tests/rtdetr_attention_ref.py) against the oracle's own
deformable_core, the heat-map helper rtdetr_decoder_heatmaps, and the argument checks of
spe_rtdetr_forward_attention and of the rt_deform_map launcher, none of which touches a device.

The GPU tolerance.  tests/test_gpu_rtdetr_attention.py compares the kernel with the float64 restatement at 4 x the
distance of the float32 restatement (the same numpy code) from the float64 one on the very inputs the kernel gets,
max over map, loc and weights.  Measured here (test_float32_restatement_distance_sets_the_gpu_tolerance prints them):
    edge-case inputs   rows 7, levels 5x3 / 2x4 / 1x1, 4 points    1.433e-07  (map 2.428e-08, loc 1.192e-07, weights 1.433e-07)
    single sample      rows 3, one 1x1 level, 1 point               1.192e-07  (loc; the weights are exactly 1)
so the gates are 5.73e-07 and 4.77e-07, absolute, on numbers of size <= 1 (map, weights) and <= 8 (loc).  The
inputs keep every location below 8: a far-away sample's fp32 ulp would otherwise be the distance.
"""
import ctypes

import numpy as np
import torch

import rtdetr_attention_ref as R
import rtdetr_ref
from spe import _lib
from spe.attention_maps import rtdetr_decoder_heatmaps
from spe.config import SpeConfig
from spe.rtdetr_spec import RtdetrConfig

N_EDGE = R.HEADS * 3 * R.EDGE_POINTS


def _edge(dtype=np.float64):
    so, ref = R.edge_case_inputs()
    return R.deform_map(so, ref, R.EDGE_Q, R.HEADS, 3, R.EDGE_POINTS, R.EDGE_LVL_H, R.EDGE_LVL_W, dtype)


def test_edge_case_inputs_cover_what_they_claim():
    so, ref = R.edge_case_inputs()
    _, loc, w, _ = _edge()
    Wl, Hl = np.asarray(R.EDGE_LVL_W, float).reshape(1, 1, 3, 1), np.asarray(R.EDGE_LVL_H, float).reshape(1, 1, 3, 1)
    ix, iy = loc[..., 0] * Wl - 0.5, loc[..., 1] * Hl - 0.5
    inside = (ix >= 0) & (ix <= Wl - 1) & (iy >= 0) & (iy <= Hl - 1)
    assert inside[list(R.ROW_INTERIOR)].all()
    e = R.ROW_EDGES
    x, y = ix[e, 0, 0], iy[e, 0, 0]                                  # head 0, level 0: one corner pair off each edge
    assert -1 < x[0] < 0 and 2 < x[1] < 3 and -1 < y[2] < 0 and 4 < y[3] < 5
    x, y = ix[e, 1, 0], iy[e, 1, 0]                                  # head 1, level 0: wholly off each edge
    assert x[0] < -1 and x[1] > 3 and y[2] < -1 and y[3] > 5
    assert ix[e, 2, 1, 0] == 2.0 and iy[e, 2, 1, 1] == 1.0           # on an integer coordinate, in fp32 too
    l32 = _edge(np.float32)[1].astype(np.float64)
    assert l32[e, 2, 1, 0, 0] * 4 - 0.5 == 2.0 and l32[e, 2, 1, 1, 1] * 2 - 0.5 == 1.0
    assert np.floor(ix[e, 2, 1, 2:]).tolist() == [1.0, 1.0] and np.floor(iy[e, 2, 1, 2:]).tolist() == [0.0, 0.0]
    assert not inside[e, 3, 2].any() and (np.abs(ix[e, 3, 2]) < 1).sum() == 2 and np.abs(loc).max() < 8
    assert inside[3:].any() and not inside[3:].all()


def test_restatement_is_the_oracles_deformable_core():
    """Per head, per_head_A @ value_h == rtdetr_ref.deformable_core(value, shapes, loc, aw) in float64: the map is
    the matrix grid_sample applies."""
    so, ref = R.edge_case_inputs()
    m, loc, w, A = _edge()
    rows, L, c = R.EDGE_ROWS, A.shape[-1], 5
    value = torch.randn(1, L, R.HEADS, c, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    shapes = list(zip(R.EDGE_LVL_H, R.EDGE_LVL_W))
    want = rtdetr_ref.deformable_core(value, shapes, torch.from_numpy(loc)[None], torch.from_numpy(w)[None])
    got = torch.einsum("qhl,lhc->qhc", torch.from_numpy(A), value[0]).reshape(1, rows, R.HEADS * c)
    assert want.abs().max() > 0.1
    assert (got - want).abs().max().item() <= 1e-12
    assert np.abs(A.mean(1) - m).max() <= 1e-15                     # the exported map is the head average


def test_single_level_restatement_is_the_oracles_deformable_core():
    so, ref = R.single_case_inputs()
    m, loc, w, A = R.deform_map(so, ref, 3, R.HEADS, 1, 1, [1], [1])
    assert (w == 1.0).all() and m.shape == (3, 1)
    value = torch.randn(1, 1, R.HEADS, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    want = rtdetr_ref.deformable_core(value, [(1, 1)], torch.from_numpy(loc)[None], torch.from_numpy(w)[None])
    got = torch.einsum("qhl,lhc->qhc", torch.from_numpy(A), value[0]).reshape(1, 3, R.HEADS * 4)
    assert (got - want).abs().max().item() <= 1e-12
    assert 0 < m[0, 0] < 1 and m[2, 0] < m[0, 0]                    # row 2 has four heads wholly off the cell


def test_rows_sum_to_at_most_one():
    m, _, w, _ = _edge()
    s = m.sum(-1)
    assert (m >= 0).all() and (s <= 1 + 1e-12).all()
    assert np.abs(s[list(R.ROW_INTERIOR)] - 1).max() <= 1e-12        # every sample interior: nothing is lost
    assert (s[R.ROW_EDGES:] < 1 - 1e-3).all()                        # mass fell off the maps
    assert np.abs(w.sum((-1, -2)) - 1).max() <= 1e-12


def test_float32_restatement_distance_sets_the_gpu_tolerance():
    """The figures of the module docstring; the kernel test's gates are 4 x these."""
    so, ref = R.edge_case_inputs()
    a, b = _edge(), _edge(np.float32)
    names = ("map", "loc", "weights")
    per = {n: float(np.abs(x - y.astype(np.float64)).max()) for n, x, y in zip(names, a, b)}
    d_edge = R.distance32(so, ref, R.EDGE_Q, R.HEADS, 3, R.EDGE_POINTS, R.EDGE_LVL_H, R.EDGE_LVL_W)
    so1, ref1 = R.single_case_inputs()
    d_single = R.distance32(so1, ref1, 3, R.HEADS, 1, 1, [1], [1])
    print(f"float32 vs float64 restatement: edge {d_edge:.3e} {per}, single {d_single:.3e}")
    assert d_edge == max(per.values())
    assert 0 < per["map"] < 1e-6 and 0 < per["weights"] < 1e-6 and 0 < d_single < 1e-6


def test_rtdetr_decoder_heatmaps():
    sizes = [4, 2, 1]
    B, Q, L = 2, 3, 21
    m = torch.zeros(B, Q, L)
    m[1, 2, 2 * 4 + 3] = 1.0                     # level 0, (y 2, x 3)
    m[0, 1, 16 + 1 * 2 + 0] = 0.5                # level 1, (y 1, x 0)
    m[0, 0, 20] = 0.25                           # level 2, its one cell
    per, comb = rtdetr_decoder_heatmaps(m, sizes)
    assert [tuple(p.shape) for p in per] == [(B, Q, 4, 4), (B, Q, 2, 2), (B, Q, 1, 1)]
    assert per[0][1, 2, 2, 3] == 1.0 and per[0].sum() == 1.0
    assert per[1][0, 1, 1, 0] == 0.5 and per[1].sum() == 0.5 and per[2][0, 0, 0, 0] == 0.25
    assert comb.shape == (B, Q, 4, 4)
    assert comb[1, 2, 2, 3] == 1.0 and comb[1, 2].sum() == 1.0
    want = torch.zeros(4, 4)
    want[2:4, 0:2] = 0.5 / 4                     # the 2 x 2 finest cells under (y 1, x 0) of level 1
    assert torch.equal(comb[0, 1], want)
    assert torch.equal(comb[0, 0], torch.full((4, 4), 0.25 / 16))
    r = torch.rand(B, Q, L, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    _, c = rtdetr_decoder_heatmaps(r, sizes)
    assert (c.sum((-1, -2)) - r.sum(-1)).abs().max() < 1e-12       # the mass is kept
    pn, cn = rtdetr_decoder_heatmaps(r.numpy(), sizes)               # numpy input
    assert torch.equal(cn, c) and pn[1].shape == (B, Q, 2, 2)


def test_oracle_capture_runs_the_oracle_model():
    """oracle_rtdetr_maps asserts its outputs equal the plain forward's; its maps have the shapes and row sums."""
    from spe.rtdetr_spec import random_rtdetr_weights
    cfg = RtdetrConfig(depth=18, input_size=64, num_queries=5, dec_layers=2)
    w = random_rtdetr_weights(cfg, 0)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    out, enc, dec, rec = R.oracle_rtdetr_maps(x, w, cfg)
    assert enc.shape == (2, 4, 4) and np.abs(enc.sum(-1) - 1).max() < 1e-12
    assert len(dec) == 2 and dec[0].shape == (2, 5, 84)
    assert all((d >= 0).all() and (d.sum(-1) <= 1 + 1e-12).all() for d in dec)
    assert not torch.equal(rec["deform"][0]["ref"], rec["deform"][1]["ref"])     # the layers' reference points differ


def _rtdetr(dtype=_lib.SPE_DTYPE_F32, dec_layers=3):
    r = RtdetrConfig(depth=18, input_size=128, dec_layers=dec_layers)
    c = _lib.RtdetrConfig(r.depth, r.input_size, r.num_queries, r.dec_layers, r.enc_ff, r.dec_ff, r.csp_hidden,
                          r.num_classes, dtype)
    h = ctypes.c_void_p()
    assert _lib.lib().spe_rtdetr_create(ctypes.byref(c), ctypes.byref(h)) == 0
    return h


def test_forward_attention_refusals_come_before_the_device():
    """Every pointer below is a dummy that is never dereferenced: each refusal comes before any launch."""
    L = _lib.lib()
    dummy = ctypes.c_void_p(16)
    out = _lib.RtdetrOutputs(dummy, dummy, *([None] * 12))

    def call(h, dl=-1, maps=(dummy, dummy, dummy, dummy), ws=dummy, images=dummy, o=out, batch=1):
        return L.spe_rtdetr_forward_attention(h, None, images, batch, ws, 1 << 40, ctypes.byref(o) if o else None, dl, *maps)

    cfg = SpeConfig(input_size=128, enc_layers=2, dec_layers=2)
    c = _lib.ModelConfig(cfg.input_size, cfg.num_queries, cfg.enc_layers, cfg.dec_layers, cfg.hidden_dim, cfg.nheads,
                         cfg.dim_feedforward, int(cfg.sigma_head), _lib.SPE_DTYPE_F32)
    d = ctypes.c_void_p()
    assert L.spe_model_create(ctypes.byref(c), ctypes.byref(d)) == 0
    assert call(d) == -1 and b"not an RT-DETR model" in L.spe_last_error()
    L.spe_model_destroy(d)

    for dt in (_lib.SPE_DTYPE_BF16, _lib.SPE_DTYPE_F32):
        h = _rtdetr(dt, dec_layers=3)
        assert call(None) == -1
        assert call(h, ws=None) == -1 and call(h, batch=0) == -1
        assert call(h, images=None) == -1 and b"null images" in L.spe_last_error()
        assert call(h, o=None) == -1 and b"null outputs" in L.spe_last_error()
        assert call(h, o=_lib.RtdetrOutputs(dummy, None, *([None] * 12))) == -1
        assert call(h, maps=(None, None, None, None)) == -1 and b"every map null" in L.spe_last_error()
        for dl in (3, -4, 7):                                        # dec_layers and -dec_layers - 1
            assert call(h, dl) == -1 and b"out of range" in L.spe_last_error(), dl
        # the order: an out-of-range layer is reported before the model's state, every map null before that
        assert call(h, 3, maps=(None, None, None, None)) == -1 and b"every map null" in L.spe_last_error()
        # in range, any one map: the call reaches the model checks (not finalized, SPE_E_STATE), still before any launch
        for dl in (0, 2, -1, -3):
            assert call(h, dl) == -2, dl
        for i in range(4):
            one = [None] * 4
            one[i] = dummy
            assert call(h, -1, maps=tuple(one)) == -2
        L.spe_model_destroy(h)


def test_deform_map_launcher_contract():
    """heads 8, 1 <= levels <= 4, 1 <= points <= 4, at most 12288 tokens, one output at least: -5 from the launcher
    before any launch (dummy pointers); no rows is 0."""
    L = _lib.lib()
    dummy = ctypes.c_void_p(16)
    five = (ctypes.c_int * 5)(2, 2, 2, 2, 2)

    def call(rows=2, heads=8, levels=3, points=4, sizes=five, outs=(dummy, dummy, dummy)):
        return L.spe_debug_rt_deform_map(None, dummy, 512, dummy, rows, 1, heads, levels, points, sizes, sizes, *outs)

    assert call(heads=4) == -5
    assert call(levels=5) == -5 and call(levels=0) == -5
    assert call(points=5) == -5 and call(points=0) == -5
    assert call(outs=(None, None, None)) == -5
    assert call(levels=1, sizes=(ctypes.c_int * 1)(111)) == -5       # 12321 tokens
    assert call(levels=2, sizes=(ctypes.c_int * 2)(0, 2)) == -5      # an empty level
    assert call(rows=0) == 0 and call(rows=-1) == 0
