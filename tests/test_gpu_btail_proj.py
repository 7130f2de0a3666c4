"""GPU: the final form of the streamed-weight bottleneck tail (btail_wide.hip) through its C ABI test hook
spe_debug_btail_wide_proj: the stride-16 model's last bottleneck conv3 (+ identity) + relu with input_proj as
the second product,

    y = relu(A . W3^T + b3 (+ R))      z = y . W1^T + b1      (no ReLU on z; y stored only when given)

at (K1, N1, N2) = (256, 1024, 256), against torch fp32 with y rounded to bf16 in between.

Tolerance, as tests/test_gpu_btail_wide.py: the inputs are pre-rounded to bf16, so only accumulation order and
the bf16 output rounding remain, max|d| <= 1e-2 * scale (scale = max|reference|, at least 1).  Y and Z start
as NaN, so an element the kernel does not write fails.  Without Y the store is the only difference: Z is
bit-identical to the run that stores Y.
"""
import ctypes

import pytest
import torch

from spe import _lib

pytestmark = pytest.mark.gpu

TOL_BF16 = 1e-2
K1, N1, N2 = 256, 1024, 256
TILE = 192                       # rows of one workgroup's tile (btail_wide.hip); one workgroup per CU


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _close(got, ref, tol):
    scale = max(1.0, ref.abs().max().item())
    err = (got.float() - ref.float()).abs().max().item()
    assert err <= tol * scale, (err, scale)


def _inputs(dev, M, res=True, pad=0, k1=K1, n1=N1, n2=N2):
    dt = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(M + k1 + n1 + n2 + pad)
    A = torch.randn(M, k1 + pad, generator=g).to(dev, dt)
    R = torch.randn(M, n1 + pad, generator=g).to(dev, dt) if res else None
    W3 = (torch.randn(n1, k1, generator=g) / k1 ** 0.5).to(dev, dt)
    b3 = (0.1 * torch.randn(n1, generator=g)).to(dev)
    W1 = (torch.randn(n2, n1, generator=g) / n1 ** 0.5).to(dev, dt)
    b1 = (0.1 * torch.randn(n2, generator=g)).to(dev)
    return A, R, W3, b3, W1, b1


def _launch(dev, inp, M, pad=0, store_y=True, relu_z=0, old_hook=False, k1=K1, n1=N1, n2=N2):
    """One launch over `inp`; returns (rc, Y or None, Z), the padded NaN-initialised buffers."""
    L = _lib.lib()
    A, R, W3, b3, W1, b1 = inp
    perm = torch.tensor([L.spe_debug_btail_wide_perm(n1, k) for k in range(n1)], device=dev)
    W1p = W1[:, perm].contiguous() if n1 in (512, 1024) else W1
    Y = torch.full((M, n1 + pad), float("nan"), dtype=torch.bfloat16, device=dev)
    Z = torch.full((M, n2 + pad), float("nan"), dtype=torch.bfloat16, device=dev)
    args = [None, _p(A), k1 + pad, k1, _p(R), n1 + pad, _p(W3), k1, _p(b3), _p(Y) if store_y else None, n1 + pad, n1,
            _p(W1p), n1, _p(b1), _p(Z), n2 + pad, n2, M]
    rc = L.spe_debug_btail_wide(*args) if old_hook else L.spe_debug_btail_wide_proj(*args, relu_z)
    torch.cuda.synchronize()
    return rc, Y, Z


def _rows(kind, cus):
    if kind == "partial":        # fewer rows than one workgroup's tile, the last 16-row fragment partial
        return 16 * 3 + 5
    if kind == "tile+19":        # one full tile and a second, partial one
        return TILE + 19
    return cus * TILE + TILE + 7  # a second round of tiles on some CUs, the last tile partial


def _check(dev, M, res=True, pad=0):
    inp = _inputs(dev, M, res, pad)
    A, R, W3, b3, W1, b1 = inp
    rc, Y, Z = _launch(dev, inp, M, pad)
    assert rc == 0, _lib.lib().spe_last_error()
    yref = torch.relu(A[:, :K1].float() @ W3.float().t() + b3 + (R[:, :N1].float() if R is not None else 0))
    _close(Y[:, :N1], yref, TOL_BF16)
    zref = Y[:, :N1].float() @ W1.float().t() + b1           # no ReLU
    assert (zref < -0.1).any() and (zref > 0.1).any()        # rows and columns whose reference z is negative
    _close(Z[:, :N2], zref, TOL_BF16)
    assert (Z[:, :N2].float() < 0).any()
    if pad:   # the columns between the rows belong to somebody else
        assert torch.isnan(Y[:, N1:]).all() and torch.isnan(Z[:, N2:]).all()
    # Y not given: nothing stored to the (unpassed) sentinel, z bit for bit the stored run's
    rc, Ysent, Z0 = _launch(dev, inp, M, pad, store_y=False)
    assert rc == 0, _lib.lib().spe_last_error()
    assert torch.isnan(Ysent).all()
    assert torch.equal(Z0[:, :N2], Z[:, :N2])
    if pad:
        assert torch.isnan(Z0[:, N2:]).all()
    return inp


@pytest.mark.parametrize("kind", ["partial", "tile+19", "second-round"])
def test_btail_proj(gpu_device, kind):
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    _check(gpu_device, _rows(kind, cus))


def test_btail_proj_without_residual(gpu_device):
    _check(gpu_device, 3 * TILE + 41, res=False)


def test_btail_proj_row_strides(gpu_device):
    _check(gpu_device, 2 * TILE + 23, pad=64)


@pytest.mark.parametrize("res", [True, False])
def test_btail_proj_relu_z_equals_the_wide_hook(gpu_device, res):
    M = TILE + 19
    inp = _inputs(gpu_device, M, res)
    rc0, Y0, Z0 = _launch(gpu_device, inp, M, old_hook=True)
    rc1, Y1, Z1 = _launch(gpu_device, inp, M, relu_z=1)
    rc2, Ysent, Z2 = _launch(gpu_device, inp, M, relu_z=1, store_y=False)
    assert rc0 == rc1 == rc2 == 0
    assert torch.equal(Z0, Z1) and torch.equal(Y0, Y1)
    assert torch.equal(Z0, Z2) and torch.isnan(Ysent).all()
    assert (Z0 >= 0).all()


# shapes this form does not serve: "not served" (1), nothing launched, nothing written
@pytest.mark.parametrize("k1,n1,n2", [(128, 512, 128), (128, 512, 256), (256, 1024, 128), (64, 512, 128)])
@pytest.mark.parametrize("store_y", [True, False])
def test_btail_proj_rejects_other_shapes(gpu_device, k1, n1, n2, store_y):
    inp = _inputs(gpu_device, 300, True, 0, k1, n1, n2)
    rc, Y, Z = _launch(gpu_device, inp, 300, store_y=store_y, k1=k1, n1=n1, n2=n2)
    assert rc == 1
    assert torch.isnan(Y).all() and torch.isnan(Z).all()
