"""GPU: the pre-norm forms of the two fused bf16 encoder kernels (csrc/ffn.hip spe_launch_ffn_pre, csrc/lnproj.hip
spe_launch_lnproj_pre) alone, through spe_debug_ffn_pre / spe_debug_oproj_pre, against torch fp32 on bf16-rounded
operands, scaled as tests/test_gpu_kernels.py's _close does."""
import ctypes

import pytest
import torch
import torch.nn.functional as F_

from spe import _lib

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _close(got, ref, tol):
    scale = max(1.0, ref.abs().max().item())
    err = (got.float() - ref.float()).abs().max().item()
    print(f"    err {err:.3e} scale {scale:.3e} bound {tol * scale:.3e}")
    assert err <= tol * scale, (err, scale)


@pytest.mark.parametrize("chunked", [0, 1])
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("M,F,splits,with_pos", [(5, 32, 0, True), (333, 2048, 0, False), (1000, 2048, 0, True),
                                                 # whole 192-row rounds + a 128-row tail launch on 256 CUs
                                                 (54152, 2048, 0, True),
                                                 (704, 2048, 16, True), (77, 128, 2, False)])
def test_ffn_pre(gpu_device, M, F, splits, with_pos, inplace, chunked):
    """n = LN(x; norm2) on chip, rounded to bf16 as a LayerNorm launch stores it; s' = x + W2 relu(W1 n + b1) + b2;
    beside it LN(s' as stored) with a second affine, and ypos = that + pos.  Bound 3e-2 x scale, test_fused_ffn's
    (hidden rounded to bf16 on chip; K = 2048 products of bf16 operands)."""
    dt, D = torch.bfloat16, 256
    dev = gpu_device
    g = torch.Generator(device="cpu").manual_seed(M + F)
    ld = D if inplace else D + 8
    x = (torch.randn(M, ld, generator=g) * 2 + 0.5).to(dev, dt)
    w1 = (torch.randn(F, D, generator=g) / D ** 0.5).to(dev, dt)
    b1 = (torch.randn(F, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(D, F, generator=g) / F ** 0.5).to(dev, dt)
    b2 = (torch.randn(D, generator=g) * 0.1).to(dev)
    gam = (torch.randn(D, generator=g) * 0.5 + 1).to(dev)
    bet = (torch.randn(D, generator=g) * 0.1).to(dev)
    gam2 = (torch.randn(D, generator=g) * 0.3 + 1.5).to(dev)      # a different affine for LN_next
    bet2 = (torch.randn(D, generator=g) * 0.2 - 0.3).to(dev)
    period = 37
    pos = torch.randn(period, D, generator=g).to(dev, dt) if with_pos else None
    xs = x[:, :D].float()
    n = F_.layer_norm(xs, (D,), gam, bet, 1e-5).to(dt).float()
    h = torch.relu(n @ w1.float().t() + b1).to(dt).float()
    s_ref = xs + h @ w2.float().t() + b2
    y = x if inplace else torch.full((M, ld), 7.0, dtype=dt, device=dev)
    y2 = torch.full((M, ld), 7.0, dtype=dt, device=dev)
    ypos = torch.full((M, ld), 7.0, dtype=dt, device=dev) if with_pos else None
    part = torch.empty(max(splits, 1), M, D, device=dev) if splits else None
    w2a, ld2 = (w2.view(D, F // 32, 32).permute(1, 0, 2).contiguous(), 0) if chunked else (w2, F)
    L = _lib.lib()
    rc = L.spe_debug_ffn_pre(None, _p(x), ld, _p(w1), D, _p(b1), _p(w2a), ld2, _p(b2), _p(gam), _p(bet), _p(y), ld, M,
                             D, F, _p(part), splits, _p(gam2), _p(bet2), _p(y2), _p(pos), period if with_pos else 0,
                             _p(ypos))
    assert rc == 0, L.spe_last_error()
    torch.cuda.synchronize()
    _close(y[:, :D], s_ref, 3e-2)
    n_ref = F_.layer_norm(s_ref, (D,), gam2, bet2, 1e-5)
    _close(y2[:, :D], n_ref, 3e-2)
    rows = torch.arange(M, device=dev) % period
    if with_pos:
        _close(ypos[:, :D], n_ref + pos.float()[rows], 3e-2)
    # LN_next is taken over s' AS STORED (what a LayerNorm launch reading y would compute): against the kernel's
    # own stored s' only the LayerNorm's bf16 output rounding is left, 2^-8 relative < 1e-2
    n_own = F_.layer_norm(y[:, :D].float(), (D,), gam2, bet2, 1e-5)
    _close(y2[:, :D], n_own, 1e-2)
    if with_pos:
        _close(ypos[:, :D], n_own + pos.float()[rows], 1e-2)
    if not inplace:
        assert (y[:, D:] == 7.0).all()                 # nothing written past column 256
    assert (y2[:, D:] == 7.0).all()
    if with_pos:
        assert (ypos[:, D:] == 7.0).all()


def test_ffn_pre_without_second_output(gpu_device):
    """y2 null: only s' is stored (the form a caller without a next LayerNorm takes)."""
    dt, D, M, F = torch.bfloat16, 256, 200, 64
    dev = gpu_device
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(M, D, generator=g).to(dev, dt)
    w1 = (torch.randn(F, D, generator=g) / 16).to(dev, dt)
    w2 = (torch.randn(D, F, generator=g) / 8).to(dev, dt)
    b1, b2 = torch.zeros(F, device=dev), torch.zeros(D, device=dev)
    gam, bet = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    y = torch.empty_like(x)
    L = _lib.lib()
    rc = L.spe_debug_ffn_pre(None, _p(x), D, _p(w1), D, _p(b1), _p(w2), F, _p(b2), _p(gam), _p(bet), _p(y), D, M, D, F,
                             None, 0, None, None, None, None, 0, None)
    assert rc == 0, L.spe_last_error()
    torch.cuda.synchronize()
    n = F_.layer_norm(x.float(), (D,), gam, bet, 1e-5).to(dt).float()
    h = torch.relu(n @ w1.float().t()).to(dt).float()
    _close(y, x.float() + h @ w2.float().t(), 3e-2)


@pytest.mark.parametrize("M", [16, 300, 256 * 256 + 77])
def test_oproj_pre(gpu_device, M):
    """s = s + ao . Wo^T + bo in place, no LayerNorm; rows off the 16-row tile, fewer tiles than waves, more tiles
    than one round of the grid.  Bound: 3e-2 x scale, test_gemm_fused_layernorm's (the lnproj test)."""
    dt, D = torch.bfloat16, 256
    dev = gpu_device
    g = torch.Generator(device="cpu").manual_seed(M)
    A = torch.randn(M, D, generator=g).to(dev, dt)
    W = (torch.randn(D, D, generator=g) / 16).to(dev, dt)
    bias = torch.randn(D, generator=g).to(dev)
    S = (torch.randn(M, D + 8, generator=g) * 3).to(dev, dt)
    ref = S[:, :D].float() + A.float() @ W.float().t() + bias
    pad = S[:, D:].clone()
    L = _lib.lib()
    rc = L.spe_debug_oproj_pre(None, _p(A), D, _p(W), D, _p(bias), _p(S), D + 8, _p(S), D + 8, M)
    assert rc == 0, L.spe_last_error()
    torch.cuda.synchronize()
    _close(S[:, :D], ref, 3e-2)
    assert torch.equal(S[:, D:], pad)
