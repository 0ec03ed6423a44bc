"""bf16 bias+GeLU forward and backward (hardware exp2 / reciprocal, packed
bf16 convert, row-strided forward) against the fp32 torch tanh-GeLU
formula, at the tolerances of test_bias_gelu.

Shapes: test_bias_gelu's (256, 512); rows 3 (fewer rows than one pass of
the grid) and 1025 (odd, one past a multiple of the rows per pass); cols
512 (one backward segment per row) and 4096 (eight segments, more than a
block's worth of vectors per row in the forward).  cols 520 and 24 leave
the backward's 512-column segment path and make the forward's threads
per row a non-divisor of the grid (idle tail threads).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from easyparallellibrary_amd import _C
else:
    _C = None


def dev():
    return torch.device("cuda:0")


def _gelu(xb):
    return 0.5 * xb * (1 + torch.tanh(0.7978845608 * (xb + 0.044715 * xb**3)))


@pytest.mark.parametrize("rows,cols", [
    (256, 512), (3, 512), (1025, 512), (256, 4096), (3, 4096), (1025, 4096),
    (1025, 520), (37, 24)])
def test_bias_gelu_bf16(rows, cols):
    torch.manual_seed(2)
    dtype = torch.bfloat16
    # a few large magnitudes: both saturated ends of the sigmoid
    x = torch.randn(rows, cols, device=dev(), dtype=dtype)
    x[0, :8] = torch.tensor([-40., -12., -6., -0., 0., 6., 12., 40.],
                            dtype=dtype)
    bias = torch.randn(cols, device=dev(), dtype=dtype)
    dy = torch.randn(rows, cols, device=dev(), dtype=dtype)
    out = torch.empty_like(x)
    _C.bias_gelu_fwd(out, x, bias)

    ref = _gelu(x.float() + bias.float())
    torch.cuda.synchronize()
    print("rows %d cols %d: fwd max |err| %.4g"
          % (rows, cols, (out.float() - ref).abs().max().item()))
    assert torch.isfinite(out.float()).all()
    assert torch.allclose(out.float(), ref, atol=2e-2, rtol=2e-2)

    dx = torch.empty_like(x)
    dbias = torch.zeros(cols, dtype=torch.float32, device=dev())
    _C.bias_gelu_bwd(dx, dbias, dy, x, bias)
    xr = x.float().clone().requires_grad_(True)
    br = bias.float().clone().requires_grad_(True)
    _gelu(xr + br).backward(dy.float())
    torch.cuda.synchronize()
    print("  bwd max |dx err| %.4g, max |dbias err| %.4g"
          % ((dx.float() - xr.grad).abs().max().item(),
             (dbias - br.grad).abs().max().item()))
    assert torch.isfinite(dx.float()).all()
    assert torch.allclose(dx.float(), xr.grad, atol=5e-2, rtol=5e-2)
    assert torch.allclose(dbias, br.grad, atol=0.5, rtol=1e-2)
