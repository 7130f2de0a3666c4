"""The RT-DETR attention maps on the GPU: the rt_deform_map kernel alone (through spe_debug_rt_deform_map) against the
float64 restatement of tests/rtdetr_attention_ref.py, its tie to msdeform (both kernels on the same operands), and
RTDETR.forward_with_attention against the oracle (oracle/rtdetr_ref.py with its attention functions wrapped).

Gates.
  kernel alone: 4 x the distance of the float32 restatement from the float64 one on the same inputs, max over map,
      loc and weights (tests/test_rtdetr_attention.py: 1.433e-07 and 1.192e-07, so 5.73e-07 and 4.77e-07); the
      margin covers the device's expf and the fused multiply-adds numpy does not have.  Measured on an MI355X
      (kernel vs float64):   edge case map 2.428e-08, loc 1.192e-07, weights 1.496e-07;   single 3.537e-08 /
      1.192e-07 / 0.
  msdeform tie: msdeform's fp32 gate of tests/test_gpu_rtdetr_kernels.py, 1e-5 max(1, max |ref|); measured 5.982e-08.
  whole model, fp32: WHOLE_FP32 below, 4 x the largest distance seen on an MI355X (dec_map 5.650e-07 at dec_layer -1,
      3.893e-07 at 0; after the 2 x 2 sums 4.186e-07 / 3.601e-07; enc_map 4.286e-08; pred_pts of the run 5.662e-07),
      and never above what the family's golden bound on pred_pts (1e-4, normalised) lets through: a reference point
      off by 1e-4 moves a sample by 1e-4 x 8 cells on the finest level of this configuration, and a cell's weight
      changes by at most that per axis, 1.6e-3.  The bilinear weights are continuous across a cell edge, so a sample
      near one moves no more mass than that; the 2 x 2 sums are reported beside the plain distance all the same.
      The exported points and weights against the oracle's records: 6.199e-06 / 8.941e-07 (the sampling offsets are a
      GEMM's output, divided by a level side of 2 at the least), gate 4 x the larger, below the 1e-4 of pred_pts.
  whole model, bf16: dec_map against the float64 splat of the exported dec_points / dec_weights at the kernel gate
      (4 x the float32 restatement's distance on those very points: 1.852e-09 against 7.406e-09); enc_map rows sum to
      1 +- 1e-5 and lie within ENC_BF16 of the fp32 model's (measured 1.424e-04 on an MI355X, the gate is 4 x that):
      no q / k export exists to recompute it from.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rtdetr_attention_ref as R
from spe import _lib
from spe.attention_maps import encoder_heatmaps_at, rtdetr_decoder_heatmaps
from spe.rtdetr import RTDETR
from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights

pytestmark = pytest.mark.gpu

NAN = float("nan")
PTS_GOLDEN_BOUND = 1e-4                      # the family's fp32 gate on pred_pts (tests/test_gpu_rtdetr_*.py)
WHOLE_FP32 = 4 * 5.650e-07                   # the measurements of the module docstring
WHOLE_FP32_POINTS = 4 * 6.199e-06            # dec_points / dec_weights against the oracle's records
ENC_BF16 = 4 * 1.424e-04


def _p(t):
    return _lib.ptr(t)


def _ints(xs):
    return (ctypes.c_int * len(xs))(*xs)


CASES = {"edge": dict(inputs=R.edge_case_inputs, Q=R.EDGE_Q, levels=3, points=R.EDGE_POINTS, lvl_h=R.EDGE_LVL_H,
                      lvl_w=R.EDGE_LVL_W),
         "single": dict(inputs=R.single_case_inputs, Q=3, levels=1, points=1, lvl_h=[1], lvl_w=[1])}


@functools.lru_cache(maxsize=None)
def _case(name):
    c = CASES[name]
    so, ref = c["inputs"]()
    args = (c["Q"], R.HEADS, c["levels"], c["points"], c["lvl_h"], c["lvl_w"])
    want = R.deform_map(so, ref, *args)
    return so, ref, want, 4.0 * R.distance32(so, ref, *args)


def _launch(dev, name, so_d, ref_d, ld_so, outs=("map", "loc", "weights")):
    """One launch over NaN-filled buffers; an output not in `outs` is passed as NULL and must keep its NaNs."""
    c = CASES[name]
    rows, n = ref_d.shape[0], R.HEADS * c["levels"] * c["points"]
    L = sum(h * w for h, w in zip(c["lvl_h"], c["lvl_w"]))
    buf = {"map": torch.full((rows, L), NAN, device=dev), "loc": torch.full((rows, n, 2), NAN, device=dev),
           "weights": torch.full((rows, n), NAN, device=dev)}
    rc = _lib.lib().spe_debug_rt_deform_map(None, _p(so_d), ld_so, _p(ref_d), rows, c["Q"], R.HEADS, c["levels"],
                                            c["points"], _ints(c["lvl_h"]), _ints(c["lvl_w"]),
                                            *[_p(buf[k]) if k in outs else None for k in ("map", "loc", "weights")])
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in buf.items()}


def _padded(so, dev):
    """so_aw rows 8 floats wider than the offsets and logits, the pad NaN"""
    t = torch.full((so.shape[0], so.shape[1] + 8), NAN)
    t[:, :so.shape[1]] = torch.from_numpy(so)
    return t.to(dev), so.shape[1] + 8


@pytest.mark.parametrize("name", list(CASES))
def test_deform_map_kernel_matches_float64(gpu_device, name):
    so, ref, (m64, loc64, w64, _), gate = _case(name)
    so_d, ld = _padded(so, gpu_device)
    ref_d = torch.from_numpy(ref).to(gpu_device)
    got = _launch(gpu_device, name, so_d, ref_d, ld)
    rows = ref.shape[0]
    err = {"map": np.abs(got["map"].double().numpy() - m64).max(),
           "loc": np.abs(got["loc"].double().numpy() - loc64.reshape(rows, -1, 2)).max(),
           "weights": np.abs(got["weights"].double().numpy() - w64.reshape(rows, -1)).max()}
    print(f"deform_map {name}: kernel vs float64 " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()) + f" (gate {gate:.3e})")
    for k, v in err.items():
        assert v <= gate, (k, v, gate)                       # (NaN fails)
    untouched = m64 == 0
    assert untouched.any() or name == "single"
    assert (got["map"].numpy()[untouched] == 0).all()        # exactly 0 where no sample has a corner
    again = _launch(gpu_device, name, so_d, ref_d, ld)
    for k in got:
        assert torch.equal(got[k], again[k]), k              # a fixed summation order: bit-identical runs
    for skip in ("map", "loc", "weights"):                   # each output left out in turn
        part = _launch(gpu_device, name, so_d, ref_d, ld, outs=[k for k in got if k != skip])
        assert torch.isnan(part[skip]).all()
        for k in got:
            if k != skip:
                assert torch.equal(part[k], got[k]), (skip, k)


def test_deform_map_is_the_matrix_msdeform_applies(gpu_device):
    """The tie between the two kernels' first step: on the same so_aw / ref, with a value whose 8 heads hold the same
    32 channels, the head mean of msdeform's output is map . value.  A drift of either kernel's softmax or sample
    positions gives errors of the order of the values."""
    dev = gpu_device
    so, ref, _, _ = _case("edge")
    rows, n = ref.shape[0], so.shape[1] // 3
    shapes = list(zip(R.EDGE_LVL_H, R.EDGE_LVL_W))
    start = np.concatenate([[0], np.cumsum([h * w for h, w in shapes])]).tolist()
    so_d, ld = _padded(so, dev)
    ref_d = torch.from_numpy(ref).to(dev)
    V = torch.randn(start[-1], 32, generator=torch.Generator().manual_seed(5))
    value = V.repeat(1, R.HEADS).contiguous().to(dev)                       # one image (Q = rows): rows0 = start
    out = torch.full((rows, 256), NAN, device=dev)
    rc = _lib.lib().spe_debug_rt_msdeform(None, _lib.SPE_DTYPE_F32, _p(value), 256, _p(so_d), ld, _p(ref_d), _p(out), 256,
                                          rows, rows, R.HEADS, 3, R.EDGE_POINTS, _ints(R.EDGE_LVL_H), _ints(R.EDGE_LVL_W),
                                          _ints(start[:-1]))
    assert rc == 0, rc
    torch.cuda.synchronize()
    m = _launch(dev, "edge", so_d, ref_d, ld)["map"].double()
    want = m @ V.double()
    got = out.cpu().double().reshape(rows, R.HEADS, 32).mean(1)
    scale = max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    print(f"msdeform head mean vs map . value: {err:.3e} (gate {1e-5 * scale:.3e}, max |ref| {scale:.2f})")
    assert want.abs().max().item() > 0.1 and err <= 1e-5 * scale


# ---------------------------------------------------------------- the whole model
CFG = RtdetrConfig(depth=18, input_size=64, num_queries=5, dec_layers=2)     # L = 84, T5 = 4
B = 2


@functools.lru_cache(maxsize=None)
def _weights():
    return random_rtdetr_weights(CFG, 0)


@functools.lru_cache(maxsize=None)
def _images():
    return torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(3))


@functools.lru_cache(maxsize=None)
def _model(dtype):
    m = RTDETR(CFG, dtype=dtype)
    m.load_state_dict(_weights())
    return m


@functools.lru_cache(maxsize=None)
def _oracle():
    return R.oracle_rtdetr_maps(_images(), _weights(), CFG)


def _flat(o, prefix=""):
    for k, v in (o.items() if isinstance(o, dict) else enumerate(o)):
        if torch.is_tensor(v):
            yield f"{prefix}{k}", v
        else:
            yield from _flat(v, f"{prefix}{k}.")


def _assert_out_is_forwards(m, x, out):
    ref = dict(_flat(m(x)))
    torch.cuda.synchronize()
    got = dict(_flat(out))
    assert list(got) == list(ref) and "aux_outputs.0.pred_pts" in got
    for k in ref:
        assert torch.equal(got[k], ref[k]), k


def _pool2(m, sizes):
    """every level's 2 x 2 neighbourhood sums (stride 1): mass that moved to a neighbouring cell cancels"""
    per, _ = rtdetr_decoder_heatmaps(torch.as_tensor(m), sizes)
    return [p if p.shape[-1] == 1 else p[..., :-1, :-1] + p[..., 1:, :-1] + p[..., :-1, 1:] + p[..., 1:, 1:] for p in per]


@pytest.mark.parametrize("dec_layer", [-1, 0])
def test_fp32_model_maps_match_the_oracle(gpu_device, dec_layer):
    m, x = _model("fp32"), _images().to(gpu_device)
    out, maps = m.forward_with_attention(x, dec_layer=dec_layer)
    torch.cuda.synchronize()
    assert maps["level_sizes"] == [8, 4, 2]
    assert maps["enc_map"].shape == (B, 4, 4) and maps["dec_map"].shape == (B, 5, 84)
    assert maps["dec_points"].shape == (B, 5, 8, 3, 4, 2) and maps["dec_weights"].shape == (B, 5, 8, 3, 4)
    _assert_out_is_forwards(m, x, out)
    o_out, enc, dec, rec = _oracle()
    want = dec[dec_layer]
    got = maps["dec_map"].double().cpu().numpy()
    d_dec = np.abs(got - want).max()
    d_pool = max((a - b).abs().max().item() for a, b in zip(_pool2(got, [8, 4, 2]), _pool2(want, [8, 4, 2])))
    d_enc = np.abs(maps["enc_map"].double().cpu().numpy() - enc).max()
    d_pts = np.abs(out["pred_pts"].cpu().numpy() - o_out["pred_pts"].numpy()).max()
    other = np.abs(got - dec[dec_layer + 1]).max()
    print(f"fp32 model vs oracle, dec_layer {dec_layer}: dec_map {d_dec:.3e} (2x2 sums {d_pool:.3e}), enc_map {d_enc:.3e}, "
          f"pred_pts {d_pts:.3e}; the other layer's map is {other:.3e} away, image 1's {np.abs(got[0] - want[1]).max():.3e}")
    # the exported points and weights against the oracle's records
    d = rec["deform"][dec_layer]
    loc = d["ref"][:, :, None, None, None, :] + d["off"] / torch.tensor([8.0, 4.0, 2.0]).reshape(1, 1, 1, 3, 1, 1)
    d_loc = (maps["dec_points"].cpu() - loc).abs().max().item()
    d_w = (maps["dec_weights"].cpu() - d["aw"]).abs().max().item()
    print(f"  dec_points {d_loc:.3e}, dec_weights {d_w:.3e}")
    cap = 2 * PTS_GOLDEN_BOUND * CFG.level_sizes[0]
    assert WHOLE_FP32 <= cap and WHOLE_FP32_POINTS <= PTS_GOLDEN_BOUND
    assert d_dec <= WHOLE_FP32 and d_enc <= WHOLE_FP32 and d_pool <= 4 * WHOLE_FP32
    assert other > 100 * WHOLE_FP32 and np.abs(got[0] - want[1]).max() > 100 * WHOLE_FP32   # a wrong layer or image shows
    assert d_loc <= WHOLE_FP32_POINTS and d_w <= WHOLE_FP32_POINTS
    # and the helpers take what the model returns
    per, comb = rtdetr_decoder_heatmaps(maps["dec_map"], maps["level_sizes"])
    assert (comb.sum((-1, -2)) - maps["dec_map"].sum(-1)).abs().max().item() <= 1e-6
    assert encoder_heatmaps_at(maps["enc_map"], out["pred_pts"], 2).shape == (B, 5, 2, 2)


def test_fp32_model_taps_can_be_skipped(gpu_device):
    m, x = _model("fp32"), _images().to(gpu_device)
    _, full = m.forward_with_attention(x)
    out, part = m.forward_with_attention(x, enc=False, points=False)
    torch.cuda.synchronize()
    assert sorted(part) == ["dec_map", "level_sizes"] and torch.equal(part["dec_map"], full["dec_map"])
    _assert_out_is_forwards(m, x, out)
    with pytest.raises(_lib.SpeError, match="out of range"):
        m.forward_with_attention(x, dec_layer=2)


def test_bf16_model_maps(gpu_device):
    m, x = _model("bf16"), _images().to(gpu_device)
    out, maps = m.forward_with_attention(x, dec_layer=-1)
    torch.cuda.synchronize()
    _assert_out_is_forwards(m, x, out)
    loc = maps["dec_points"].double().cpu().numpy().reshape(B * 5, 8, 3, 4, 2)
    w = maps["dec_weights"].double().cpu().numpy().reshape(B * 5, 8, 3, 4)
    assert np.abs(w.sum((-1, -2)) - 1).max() <= 1e-6
    sizes = [8, 4, 2]
    want, _ = R.splat(loc, w, sizes, sizes)
    own, _ = R.splat(loc.astype(np.float32), w.astype(np.float32), sizes, sizes)
    gate = 4.0 * np.abs(own.astype(np.float64) - want).max()
    d = np.abs(maps["dec_map"].double().cpu().numpy().reshape(B * 5, -1) - want).max()
    print(f"bf16 model: dec_map vs the float64 splat of its own points {d:.3e} (gate {gate:.3e})")
    assert d <= gate
    enc = maps["enc_map"].cpu()
    assert (enc.sum(-1) - 1).abs().max().item() <= 1e-5 and (enc >= 0).all()
    _, f32 = _model("fp32").forward_with_attention(x)
    d_enc = (enc - f32["enc_map"].cpu()).abs().max().item()
    print(f"bf16 model: enc_map vs the fp32 model's {d_enc:.3e}")
    assert ENC_BF16 is not None and d_enc <= ENC_BF16


def test_mobilenetv3_small_backbone_shapes_and_row_sums(gpu_device):
    cfg = RtdetrConfig(backbone="MobileNetV3_Small", input_size=256)
    m = RTDETR(cfg, dtype="bf16")
    m.load_state_dict(random_rtdetr_weights(cfg, 0))
    x = torch.randn(1, 3, 256, 256, generator=torch.Generator().manual_seed(4)).to(gpu_device)
    out, maps = m.forward_with_attention(x)
    torch.cuda.synchronize()
    Q, L = cfg.num_queries, 32 * 32 + 16 * 16 + 8 * 8
    assert maps["level_sizes"] == [32, 16, 8]
    assert maps["enc_map"].shape == (1, 64, 64) and maps["dec_map"].shape == (1, Q, L)
    assert maps["dec_points"].shape == (1, Q, 8, 3, 4, 2) and maps["dec_weights"].shape == (1, Q, 8, 3, 4)
    assert (maps["enc_map"].sum(-1) - 1).abs().max().item() <= 1e-5
    s = maps["dec_map"].sum(-1)
    assert (maps["dec_map"] >= 0).all() and (s <= 1 + 1e-5).all() and s.max().item() > 0.5
    assert (maps["dec_weights"].sum((-1, -2)) - 1).abs().max().item() <= 1e-5
    _assert_out_is_forwards(m, x, out)
