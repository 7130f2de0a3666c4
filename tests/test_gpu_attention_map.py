"""GPU: the attention-map kernel (csrc/attn_map.hip) through spe_debug_attn_map, and
spe_forward_attention / DETR.forward_with_attention against the oracle model's maps.

Bounds.  Every gate is 4 x the max abs difference between the torch-fp32 CPU restatement and the fp64 one
on the same inputs (the kernel sums in another order than torch); the spread is computed by the test on its
seeded inputs and printed with the kernel's error.  Measured on MI355X (spread -> kernel error, bound = 4 x
spread):
  kernel, fp32 / bf16 inputs   see KERNEL_MEASURED below
  model fp32, S = 128 / 160    see MODEL_MEASURED below
"""
import pytest
import torch

import attention_map_ref as R
from spe import _lib
from spe.config import SpeConfig
from spe.synthetic import random_weights, synthetic_batch

pytestmark = pytest.mark.gpu

# (Tq, Tk): full tiles, a 16-column tail, few rows, the decoder's shape at 224^2 / 40 queries, a one-column tail
KERNEL_SHAPES = [(256, 256), (400, 400), (11, 400), (40, 784), (1, 65)]
GUARD = 64            # floats on each side of `out`
FILL = -7.0
# measured on MI355X, max abs over the map: {(Tq, Tk, dtype): (fp32-vs-fp64 spread, kernel error vs fp64)}
KERNEL_MEASURED = {
    (256, 256, "fp32"): (1.594e-07, 1.867e-07),
    (256, 256, "bf16"): (1.802e-07, 8.372e-08),
    (256, 256, "fp16"): (1.305e-07, 7.707e-08),
    (400, 400, "fp32"): (1.663e-07, 1.801e-07),
    (400, 400, "bf16"): (1.597e-07, 7.236e-08),
    (400, 400, "fp16"): (1.802e-07, 8.429e-08),
    (11, 400, "fp32"): (1.027e-07, 1.078e-07),
    (11, 400, "bf16"): (1.038e-07, 4.554e-08),
    (11, 400, "fp16"): (9.046e-08, 5.959e-08),
    (40, 784, "fp32"): (1.561e-07, 1.525e-07),
    (40, 784, "bf16"): (1.409e-07, 6.735e-08),
    (40, 784, "fp16"): (1.211e-07, 7.613e-08),
    (1, 65, "fp32"): (5.821e-08, 7.521e-08),
    (1, 65, "bf16"): (3.960e-08, 3.491e-08),
    (1, 65, "fp16"): (3.903e-08, 3.401e-08),
    (11, 400, "bf16 folded"): (4.740e-08, 5.188e-08),
}
# {(input_size, "enc0" | "enc1" | "dec0" | "dec1"): (oracle fp32-vs-fp64 spread, HIP fp32 model error vs the fp64 oracle)}
MODEL_MEASURED = {
    (128, "dec0"): (2.642e-09, 6.522e-09),
    (128, "dec1"): (2.800e-09, 7.000e-09),
    (128, "enc0"): (7.636e-08, 1.876e-07),
    (128, "enc1"): (4.039e-09, 9.076e-09),
    (160, "dec0"): (1.618e-09, 3.985e-09),
    (160, "dec1"): (1.792e-09, 4.007e-09),
    (160, "enc0"): (9.178e-08, 1.926e-07),
    (160, "enc1"): (1.883e-09, 4.785e-09),
}

_DT = {"fp32": (_lib.SPE_DTYPE_F32, torch.float32), "bf16": (_lib.SPE_DTYPE_BF16, torch.bfloat16),
       "fp16": (_lib.SPE_DTYPE_F16, torch.float16)}


def _run_kernel(q, k, code, Tq, Tk, dev, stream=None):
    """spe_debug_attn_map into the middle of a filled buffer; returns the map and checks the guard bands."""
    B = q.shape[0]
    n = B * Tq * Tk
    buf = torch.full((n + 2 * GUARD,), FILL, device=dev)
    out = buf[GUARD:GUARD + n]
    _lib.check(_lib.lib().spe_debug_attn_map(_lib.stream_ptr(stream), _lib.ptr(q), _lib.ptr(k), B, 8, Tq, Tk, code,
                                             _lib.ptr(out)), "spe_debug_attn_map")
    torch.cuda.synchronize()
    host = buf.cpu()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + n:] == FILL).all(), "wrote outside [B,Tq,Tk]"
    return host[GUARD:GUARD + n].view(B, Tq, Tk)


_kernel_refs = {}


def _kernel_ref(Tq, Tk, dtype):
    """(q, k) rounded to the storage type, the fp64 restatement of those values and the fp32 one's spread"""
    key = (Tq, Tk, dtype)
    if key not in _kernel_refs:
        q, k = R.kernel_case(Tq, Tk, seed=Tq * 1000 + Tk, sigma=2.1)
        q, k = q.to(_DT[dtype][1]), k.to(_DT[dtype][1])
        r64 = R.head_avg_probs(q.double(), k.double())
        spread = (R.head_avg_probs(q.float(), k.float()).double() - r64).abs().max().item()
        _kernel_refs[key] = (q, k, r64, spread)
    return _kernel_refs[key]


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("Tq,Tk", KERNEL_SHAPES)
def test_kernel_matches_fp64_restatement(gpu_device, Tq, Tk, dtype):
    q, k, r64, spread = _kernel_ref(Tq, Tk, dtype)
    got = _run_kernel(q.to(gpu_device).contiguous(), k.to(gpu_device).contiguous(), _DT[dtype][0], Tq, Tk, gpu_device)
    err = (got.double() - r64).abs().max().item()
    rows = (got.double().sum(-1) - 1).abs().max().item()
    print(f"attn_map kernel {dtype} ({Tq},{Tk}): spread {spread:.3e} error {err:.3e} bound {4 * spread:.3e} "
          f"row-sum error {rows:.3e}")
    assert torch.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    assert rows <= 1e-5
    assert err <= 4 * spread


def test_kernel_folded_decoder_form(gpu_device):
    """The bf16 decoder's operands (xattn.hip): q' [B,Q,8*256] in the exp2 domain against one k [B,T,256];
    256-wide heads, scores about +-20 in log2 units.  Same rule for the bound."""
    B, Q, T = 2, 11, 400
    g = torch.Generator().manual_seed(5)
    qf = (torch.randn(B, Q, 8 * 256, generator=g) * 0.55).bfloat16()
    k = (torch.randn(B, T, 256, generator=g) * 0.55).bfloat16()
    r64 = R.head_avg_probs_folded(qf.double(), k.double())
    spread = (R.head_avg_probs_folded(qf.float(), k.float()).double() - r64).abs().max().item()
    got = _run_kernel(qf.to(gpu_device), k.to(gpu_device), _lib.SPE_DTYPE_BF16 | 0x100, Q, T, gpu_device)
    err = (got.double() - r64).abs().max().item()
    print(f"attn_map kernel folded bf16 ({Q},{T}): spread {spread:.3e} error {err:.3e} bound {4 * spread:.3e}")
    assert (got >= 0).all() and (got <= 1).all() and (got.double().sum(-1) - 1).abs().max() <= 1e-5
    assert err <= 4 * spread


def test_kernel_batch_independence_and_stream(gpu_device):
    """Image 1 of a B = 3 launch equals the B = 1 launch on its operands bit for bit, also on another stream."""
    Tq, Tk = 40, 400
    q, k = R.kernel_case(Tq, Tk, seed=9, B=3, sigma=2.1)
    q, k = q.to(gpu_device), k.to(gpu_device)
    full = _run_kernel(q, k, _lib.SPE_DTYPE_F32, Tq, Tk, gpu_device)
    s = torch.cuda.Stream(gpu_device)
    s.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(s):
        one = _run_kernel(q[1:2].contiguous(), k[1:2].contiguous(), _lib.SPE_DTYPE_F32, Tq, Tk, gpu_device, stream=s)
    assert torch.equal(full[1:2], one)


# ---------------------------------------------------------------- model level
_models, _oracles = {}, {}


def _cfg(S):
    return SpeConfig(input_size=S, enc_layers=2, dec_layers=2)


def _model(S, dtype, attn_dtype=None):
    from spe.models import DETR
    key = (S, dtype, attn_dtype)
    if key not in _models:
        m = DETR(_cfg(S), dtype=dtype, attn_dtype=attn_dtype)
        m.load_state_dict(random_weights(_cfg(S), 7))
        _models[key] = m
    return _models[key]


def _batch(S, B, dev):
    b = synthetic_batch(_cfg(S), B, 123)
    return torch.from_numpy(b["images"]).to(dev), torch.from_numpy(b["clip_bbox"]).float().to(dev)


def _oracle(S):
    """The oracle model's maps of every layer on the B = 2 batch, in fp32 and fp64 (computed once)."""
    if S not in _oracles:
        cfg = _cfg(S)
        b = synthetic_batch(cfg, 2, 123)
        w = random_weights(cfg, 7)
        with torch.no_grad():
            _, e32, d32 = R.oracle_attention_maps(b["images"], w, cfg)
            _, e64, d64 = R.oracle_attention_maps(b["images"], w, cfg, torch.float64)
        _oracles[S] = {"enc": (e32, e64), "dec": (d32, d64)}
    return _oracles[S]


def _same_outputs(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("S", [128, 160])        # T = 256 (full tiles), T = 400 (a 16-column tail)
def test_model_fp32_maps_match_oracle(gpu_device, S):
    m = _model(S, "fp32")
    img, clip = _batch(S, 2, gpu_device)
    ref = m(img, clip_bbox=clip)
    ora = _oracle(S)
    maps = {}
    for el, dl in ((-1, -2), (0, -1)):           # the reference's layers, then the other two
        out, mp = m.forward_with_attention(img, enc_layer=el, dec_layer=dl, clip_bbox=clip)
        torch.cuda.synchronize()
        _same_outputs(out, ref)                  # the regular outputs: forward()'s, bit for bit
        maps[f"enc{el % 2}"], maps[f"dec{dl % 2}"] = mp["enc"].cpu(), mp["dec"].cpu()
    T, Q = (S // 8) ** 2, 11
    assert maps["enc0"].shape == (2, T, T) and maps["dec0"].shape == (2, Q, T)
    assert not torch.equal(maps["enc0"], maps["enc1"])
    fails = []
    for name, got in maps.items():
        o32, o64 = (x[int(name[3])] for x in ora[name[:3]])
        spread = (o32.double() - o64).abs().max().item()
        err = (got.double() - o64).abs().max().item()
        err32 = (got - o32).abs().max().item()
        print(f"attn_map model fp32 S={S} {name}: oracle spread {spread:.3e} error vs fp64 oracle {err:.3e} "
              f"(vs fp32 oracle {err32:.3e}) bound {4 * spread:.3e} map max {o64.max().item():.3e}")
        assert (got.double().sum(-1) - 1).abs().max() <= 1e-5 and (got >= 0).all()
        if err > 4 * spread:
            fails.append((name, err, 4 * spread))
    # each layer matches ITS oracle layer, far closer than the two layers are to each other
    assert (maps["enc0"].double() - ora["enc"][1][0]).abs().max() < 0.01 * (ora["enc"][1][0] - ora["enc"][1][1]).abs().max()
    assert (maps["enc1"].double() - ora["enc"][1][1]).abs().max() < 0.01 * (ora["enc"][1][0] - ora["enc"][1][1]).abs().max()
    assert not fails, fails


@pytest.mark.parametrize("attn_dtype", [None, "fp16"])
def test_model_bf16_maps(gpu_device, attn_dtype):
    S = 160
    m = _model(S, "bf16", attn_dtype)
    img, clip = _batch(S, 2, gpu_device)
    ref = m(img, clip_bbox=clip)
    out, mp = m.forward_with_attention(img, clip_bbox=clip)
    torch.cuda.synchronize()
    _same_outputs(out, ref)
    _, mp32 = _model(S, "fp32").forward_with_attention(img, clip_bbox=clip)
    for name in ("enc", "dec"):
        got = mp[name].cpu()
        assert torch.isfinite(got).all() and (got >= 0).all()
        assert (got.double().sum(-1) - 1).abs().max() <= 1e-3
        print(f"attn_map model bf16 attn_dtype={attn_dtype} S={S} {name}: mean abs difference to the fp32-mode map "
              f"{(got - mp32[name].cpu()).abs().mean().item():.3e} (map mean {1.0 / got.shape[-1]:.3e})")


def test_model_one_null_map(gpu_device):
    S = 128
    m = _model(S, "fp32")
    img, _ = _batch(S, 2, gpu_device)
    _, both = m.forward_with_attention(img)
    T = (S // 8) ** 2
    for skip, keep in (("enc", "dec"), ("dec", "enc")):
        # spe_forward_attention gets NULL for `skip`: the other map is unchanged, and the buffer that held
        # the skipped map in the two-map call keeps its fill pattern
        bufs = {"enc": torch.full((2, T, T), FILL, device=gpu_device), "dec": torch.full((2, 11, T), FILL, device=gpu_device)}
        _, mp = m.forward_with_attention(img, maps={skip: None, keep: bufs[keep]})
        torch.cuda.synchronize()
        assert list(mp) == [keep] and torch.equal(bufs[keep], both[keep])
        assert (bufs[skip] == FILL).all()


def test_model_non_default_stream(gpu_device):
    S = 128
    m = _model(S, "fp32")
    img, clip = _batch(S, 2, gpu_device)
    out0, mp0 = m.forward_with_attention(img, clip_bbox=clip)
    s = torch.cuda.Stream(gpu_device)
    s.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(s):
        out1, mp1 = m.forward_with_attention(img, clip_bbox=clip, stream=s)
    s.synchronize()
    torch.cuda.synchronize()
    _same_outputs(out0, out1)
    assert torch.equal(mp0["enc"], mp1["enc"]) and torch.equal(mp0["dec"], mp1["dec"])


def test_model_batch_independence(gpu_device):
    """The B = 1 maps equal image 1's rows of the B = 3 maps bit for bit."""
    S = 128
    m = _model(S, "fp32")
    img, _ = _batch(S, 3, gpu_device)
    _, full = m.forward_with_attention(img)
    _, one = m.forward_with_attention(img[1:2].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(full["enc"][1:2], one["enc"]) and torch.equal(full["dec"][1:2], one["dec"])
