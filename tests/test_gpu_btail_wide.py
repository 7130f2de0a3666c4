"""GPU: the streamed-weight bottleneck tail (btail_wide.hip) through its C ABI test hook: the
layer-2 / layer-3 conv3 (+ identity) + relu fused with the next block's conv1 + relu,

    y = relu(A . W3^T + b3 (+ R))      z = relu(y . W1^T + b1)

against torch fp32 of the two convs with y rounded to bf16 in between (the separate launches'
intermediate): Y against the fp32 product, Z against the product of the KERNEL's bf16 Y.

Tolerance, as for the layer-1 kernel: the inputs are pre-rounded to bf16, so only accumulation
order and the bf16 output rounding remain, max|d| <= 1e-2 * scale (scale = max|reference|, at
least 1).  Y and Z start as NaN, so an element the kernel does not write fails.
"""
import ctypes

import pytest
import torch

from spe import _lib

pytestmark = pytest.mark.gpu

TOL_BF16 = 1e-2
SHAPES = [(128, 512, 128), (128, 512, 256), (256, 1024, 256)]   # (K1, N1, N2)
# rows of one workgroup's tile, and workgroups resident per CU (btail_wide.hip): the row counts
# below are placed around them
TILE_ROWS = {512: 128, 1024: 192}
WG_PER_CU = {(128, 512, 128): 2, (128, 512, 256): 1, (256, 1024, 256): 1}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _close(got, ref, tol):
    scale = max(1.0, ref.abs().max().item())
    err = (got.float() - ref.float()).abs().max().item()
    assert err <= tol * scale, (err, scale)


def _perm(L, n1, dev):
    perm = [L.spe_debug_btail_wide_perm(n1, k) for k in range(n1)]
    assert sorted(perm) == list(range(n1))
    return torch.tensor(perm, device=dev)


def _run(dev, M, k1, n1, n2, res=True, pad=0):
    """Launches the hook on fresh inputs (row strides `pad` elements wider than the rows) and
    returns (rc, A, R, W3, b3, W1, b1, Y, Z) with Y / Z the padded buffers."""
    L = _lib.lib()
    dt = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(M + k1 + n1 + n2 + pad)
    A = torch.randn(M, k1 + pad, generator=g).to(dev, dt)
    R = torch.randn(M, n1 + pad, generator=g).to(dev, dt) if res else None
    W3 = (torch.randn(n1, k1, generator=g) / k1 ** 0.5).to(dev, dt)
    b3 = (0.1 * torch.randn(n1, generator=g)).to(dev)
    W1 = (torch.randn(n2, n1, generator=g) / n1 ** 0.5).to(dev, dt)
    b1 = (0.1 * torch.randn(n2, generator=g)).to(dev)
    W1p = W1[:, _perm(L, n1, dev)].contiguous() if n1 in TILE_ROWS else W1
    Y = torch.full((M, n1 + pad), float("nan"), dtype=dt, device=dev)
    Z = torch.full((M, n2 + pad), float("nan"), dtype=dt, device=dev)
    rc = L.spe_debug_btail_wide(None, _p(A), k1 + pad, k1, _p(R), n1 + pad, _p(W3), k1, _p(b3), _p(Y), n1 + pad, n1,
                                _p(W1p), n1, _p(b1), _p(Z), n2 + pad, n2, M)
    torch.cuda.synchronize()
    return rc, A, R, W3, b3, W1, b1, Y, Z


def _check(M, k1, n1, n2, out, pad=0):
    rc, A, R, W3, b3, W1, b1, Y, Z = out
    assert rc == 0, _lib.lib().spe_last_error()
    yref = torch.relu(A[:, :k1].float() @ W3.float().t() + b3 + (R[:, :n1].float() if R is not None else 0))
    _close(Y[:, :n1], yref, TOL_BF16)
    zref = torch.relu(Y[:, :n1].float() @ W1.float().t() + b1)
    _close(Z[:, :n2], zref, TOL_BF16)
    if pad:   # the columns between the rows belong to somebody else
        assert torch.isnan(Y[:, n1:]).all() and torch.isnan(Z[:, n2:]).all()


def _rows(kind, k1, n1, n2, cus):
    tile = TILE_ROWS[n1]
    if kind == "partial":        # fewer rows than one workgroup's tile, the last 16-row fragment partial
        return 16 * 3 + 5
    if kind == "tile+19":        # one full tile and a second, partial one
        return tile + 19
    # more tiles than the chip holds at once, so some CUs take a second one; the last tile partial
    return cus * WG_PER_CU[(k1, n1, n2)] * tile + tile + 7


@pytest.mark.parametrize("kind", ["partial", "tile+19", "second-round"])
@pytest.mark.parametrize("k1,n1,n2", SHAPES)
def test_btail_wide(gpu_device, k1, n1, n2, kind):
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    M = _rows(kind, k1, n1, n2, cus)
    _check(M, k1, n1, n2, _run(gpu_device, M, k1, n1, n2))


def test_btail_wide_without_residual(gpu_device):
    k1, n1, n2 = SHAPES[0]
    M = 3 * TILE_ROWS[n1] + 41
    _check(M, k1, n1, n2, _run(gpu_device, M, k1, n1, n2, res=False))


# block 6 writes its output into a buffer that the neck reads later: row strides wider than the rows
@pytest.mark.parametrize("k1,n1,n2", [SHAPES[1], SHAPES[2]])
def test_btail_wide_row_strides(gpu_device, k1, n1, n2):
    M = 2 * TILE_ROWS[n1] + 23
    _check(M, k1, n1, n2, _run(gpu_device, M, k1, n1, n2, pad=64), pad=64)


# a shape the kernel does not serve: "not served" (1), nothing launched, nothing written
@pytest.mark.parametrize("k1,n1,n2", [(64, 512, 128), (128, 256, 128), (256, 1024, 128)])
def test_btail_wide_rejects_other_shapes(gpu_device, k1, n1, n2):
    rc, *_, Y, Z = _run(gpu_device, 300, k1, n1, n2)
    assert rc == 1
    assert torch.isnan(Y).all() and torch.isnan(Z).all()


@pytest.mark.parametrize("n1", [512, 1024])
def test_btail_wide_perm_is_a_permutation(gpu_device, n1):
    L = _lib.lib()
    _perm(L, n1, gpu_device)
    assert L.spe_debug_btail_wide_perm(n1, n1) == -1 and L.spe_debug_btail_wide_perm(n1, -1) == -1
