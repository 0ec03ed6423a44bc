"""LayerNorm backward with the in-kernel dadd / colsum fusions, against the
fp32 torch LayerNorm backward (the reference of test_layer_norm_fwd_bwd):

    dx_ref     = LNbwd(dy) + dadd.float()
    colsum_ref = dx_ref.sum(0)

Tolerances are that test's: dx atol=rtol=5e-2, colsum the dbeta tolerance
(atol 0.5, rtol 1e-2), dgamma/dbeta unchanged.
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


# cols 512 / 1024 / 2048: CHUNKS = 1 / 2 / 4; 1600: CHUNKS = 4 with a
# masked column tail.  rows 3: most waves own no row and must write zero
# partials; rows 8191: odd, and more rows than resident waves (the
# grid-stride loop runs twice).
SHAPES = [(512, 64), (1024, 64), (1600, 64), (2048, 64), (1024, 3),
          (1024, 8191), (512, 8191), (1600, 8191)]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]

_cache = {}


def _case(cols, rows):
    """Inputs, forward statistics and the fp32 references, built once per
    shape and shared (read-only) by the flag combinations."""
    key = (cols, rows)
    if key in _cache:
        return _cache[key]
    g = torch.Generator(device="cpu").manual_seed(cols * 10007 + rows)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev(), torch.bfloat16)

    x, dy, dadd = rnd(rows, cols), rnd(rows, cols), rnd(rows, cols)
    gamma, beta = rnd(cols), rnd(cols)
    mean = torch.empty(rows, dtype=torch.float32, device=dev())
    rstd = torch.empty(rows, dtype=torch.float32, device=dev())
    out = torch.empty_like(x)
    _C.layer_norm_fwd(out, x, None, None, gamma, beta, mean, rstd, 1e-5)

    xr = x.float().clone().requires_grad_(True)
    gr = gamma.float().clone().requires_grad_(True)
    br = beta.float().clone().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (cols,), gr, br, 1e-5)
    ref.backward(dy.float())
    c = dict(x=x, dy=dy, dadd=dadd, gamma=gamma, mean=mean, rstd=rstd,
             dx_ln=xr.grad.detach(), dgamma=gr.grad.detach(),
             dbeta=br.grad.detach())
    _cache[key] = c
    return c


def _run(c, fn, *extra):
    cols = c["x"].shape[1]
    dx = torch.empty_like(c["x"])
    dgamma = torch.zeros(cols, dtype=torch.float32, device=dev())
    dbeta = torch.zeros(cols, dtype=torch.float32, device=dev())
    fn(dx, dgamma, dbeta, c["dy"], c["x"], c["gamma"], c["mean"], c["rstd"],
       *extra)
    return dx, dgamma, dbeta


@pytest.mark.parametrize("use_dadd,use_colsum", FLAGS)
@pytest.mark.parametrize("cols,rows", SHAPES)
def test_ln_bwd_fused_kernel(cols, rows, use_dadd, use_colsum):
    c = _case(cols, rows)
    colsum = (torch.zeros(cols, dtype=torch.float32, device=dev())
              if use_colsum else None)
    dx, dgamma, dbeta = _run(c, _C.layer_norm_bwd_fused,
                             c["dadd"] if use_dadd else None, colsum)
    torch.cuda.synchronize()
    dx_ref = c["dx_ln"] + c["dadd"].float() if use_dadd else c["dx_ln"]
    err = (dx.float() - dx_ref).abs().max().item()
    print("cols %d rows %d dadd %d colsum %d: max |dx err| %.4g"
          % (cols, rows, use_dadd, use_colsum, err))
    assert torch.allclose(dx.float(), dx_ref, atol=5e-2, rtol=5e-2)
    assert torch.allclose(dgamma, c["dgamma"], atol=0.5, rtol=1e-2)
    assert torch.allclose(dbeta, c["dbeta"], atol=0.5, rtol=1e-2)
    if use_colsum:
        cs_ref = dx_ref.sum(0)
        print("  max |colsum err| %.4g"
              % (colsum - cs_ref).abs().max().item())
        assert torch.allclose(colsum, cs_ref, atol=0.5, rtol=1e-2)


@pytest.mark.parametrize("cols,rows", SHAPES)
def test_ln_bwd_fused_none_equals_plain(cols, rows):
    """Neither flag: the same bits as layer_norm_bwd.  dx has one writer
    per element and must match exactly.  dgamma/dbeta are summed by 64
    fp32 atomicAdds per column whose order the hardware picks, in both
    entry points alike, so two runs of the SAME entry point may already
    differ in the last bits; they are held to the fp32 reassociation error of
    that sum: each order is within 63 * 2^-24 * sum |addend| of the exact
    sum, so two orders are within 128 * 2^-24 * sum |addend| of each
    other, and sum |dy * xhat| over the rows bounds sum |addend|."""
    c = _case(cols, rows)
    dx0, dg0, db0 = _run(c, _C.layer_norm_bwd)
    dx1, dg1, db1 = _run(c, _C.layer_norm_bwd_fused, None, None)
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1)
    xhat = (c["x"].float() - c["mean"][:, None]) * c["rstd"][:, None]
    bound_g = 128 * 2.0 ** -24 * (c["dy"].float() * xhat).abs().sum(0)
    bound_b = 128 * 2.0 ** -24 * c["dy"].float().abs().sum(0)
    assert ((dg0 - dg1).abs() <= bound_g).all()
    assert ((db0 - db1).abs() <= bound_b).all()


@pytest.mark.parametrize("dtype,cols", [(torch.float32, 1024),
                                        (torch.bfloat16, 4096)])
def test_ln_bwd_fused_fallback_shapes(dtype, cols):
    """fp32 and cols > 2048 have no fused kernel: the binding refuses the
    optional arguments there, and the Python entry gives the same dx and
    colsum through the separate add and sum."""
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.ops.layer_norm import layer_norm_bwd_fused
    epl.init()
    torch.manual_seed(5)
    rows = 64
    x = torch.randn(rows, cols, device=dev(), dtype=dtype)
    dy = torch.randn(rows, cols, device=dev(), dtype=dtype)
    dadd = torch.randn(rows, cols, device=dev(), dtype=dtype)
    gamma = torch.randn(cols, device=dev(), dtype=dtype)
    beta = torch.randn(cols, device=dev(), dtype=dtype)
    mean = torch.empty(rows, dtype=torch.float32, device=dev())
    rstd = torch.empty(rows, dtype=torch.float32, device=dev())
    out = torch.empty_like(x)
    _C.layer_norm_fwd(out, x, None, None, gamma, beta, mean, rstd, 1e-5)

    dx0 = torch.empty_like(x)
    dgamma = torch.zeros(cols, dtype=torch.float32, device=dev())
    dbeta = torch.zeros(cols, dtype=torch.float32, device=dev())
    with pytest.raises(RuntimeError):
        _C.layer_norm_bwd_fused(dx0, dgamma, dbeta, dy, x, gamma, mean, rstd,
                                dadd, None)

    dx, dgamma, dbeta, colsum = layer_norm_bwd_fused(
        dy, x, gamma, mean, rstd, dadd=dadd, want_colsum=True)
    xr = x.float().clone().requires_grad_(True)
    gr = gamma.float().clone().requires_grad_(True)
    br = beta.float().clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (cols,), gr, br, 1e-5).backward(
        dy.float())
    dx_ref = xr.grad + dadd.float()
    torch.cuda.synchronize()
    tol = 5e-2 if dtype == torch.bfloat16 else 1e-4
    assert torch.allclose(dx.float(), dx_ref, atol=tol, rtol=tol)
    assert torch.allclose(colsum, dx_ref.sum(0), atol=0.5, rtol=1e-2)
    assert torch.allclose(dgamma, gr.grad, atol=0.5, rtol=1e-2)
    assert torch.allclose(dbeta, br.grad, atol=0.5, rtol=1e-2)


# ---- module level: Block in bf16 on the GPU vs fp32 on the CPU -------------

def _block_run(pre_ln, device, dtype, state, x, w):
    from easyparallellibrary_amd.models.transformer import Block
    blk = Block(128, 2, 512, causal=pre_ln, pre_ln=pre_ln)
    blk.load_state_dict(state)
    blk = blk.to(device, dtype)
    xi = x.detach().clone().to(device, dtype).requires_grad_(True)
    y = blk(xi)
    (y.float() * w.to(device)).sum().backward()
    grads = {n: p.grad.float().cpu() for n, p in blk.named_parameters()}
    return y.float().cpu(), xi.grad.float().cpu(), grads


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("pre_ln", [False, True])
def test_block_bf16_matches_fp32_cpu(pre_ln, fuse, monkeypatch):
    """Block (hidden 128, seq 64, batch 2) in bf16 with the LN-backward
    fusion on and off, each against the fp32 CPU run of the same weights,
    at the tolerances of test_fused_residual_layer_norm_gpu
    (atol = rtol = 5e-2).

    Those tolerances have an absolute part, so the loss fixes what they
    mean.  The upstream gradient is randn / sqrt(rows): parameter
    gradients (sums over the 128 rows) then come out O(1), the scale that
    test's randn activations have.  With a plain randn upstream they are
    O(10-30), where bf16's own spacing (0.125) and the rounding noise of
    a 128-term bf16 sum already exceed 5e-2 for the unfused path too
    (measured: ln1.weight max error 0.115 at max |ref| 30.7, fusion on
    and off alike).

    Because the input gradient is then O(0.1), where 5e-2 absolute says
    little, every gradient is also held to a relative L2 error of 2e-2:
    each passes through at most ~16 bf16 roundings of 2^-9 relative
    size, independent, so about sqrt(16) * 2^-9 = 0.8 % is expected,
    while a dropped term (the ds add, a bias gradient) is an O(1)
    relative error."""
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models.transformer import (Block,
                                                            init_weights)
    from easyparallellibrary_amd.ops import layer_norm
    epl.init()
    torch.manual_seed(11)
    src = init_weights(Block(128, 2, 512, causal=pre_ln, pre_ln=pre_ln))
    with torch.no_grad():
        for n, p in src.named_parameters():
            if n.endswith("bias"):
                p.normal_(std=0.02)
    # weights exactly representable in bf16, so both runs see the same
    state = {k: v.to(torch.bfloat16).float()
             for k, v in src.state_dict().items()}
    x = torch.randn(2, 64, 128).to(torch.bfloat16).float()
    w = torch.randn(2, 64, 128) / (2 * 64) ** 0.5

    monkeypatch.setattr(layer_norm, "_LN_BWD_FUSE", False)
    y_ref, dx_ref, g_ref = _block_run(pre_ln, "cpu", torch.float32, state,
                                      x, w)
    monkeypatch.setattr(layer_norm, "_LN_BWD_FUSE", fuse)
    y, dx, g = _block_run(pre_ln, dev(), torch.bfloat16, state, x, w)

    def rel(a, b):
        return ((a - b).norm() / b.norm()).item()

    tol = 5e-2
    assert list(g) == list(g_ref)
    print("pre_ln %d fuse %d dx: max |err| %.4g (max |ref| %.4g) rel L2 %.4g"
          % (pre_ln, fuse, (dx - dx_ref).abs().max().item(),
             dx_ref.abs().max().item(), rel(dx, dx_ref)))
    for n in g_ref:
        print("pre_ln %d fuse %d %s: max |err| %.4g (max |ref| %.4g) "
              "rel L2 %.4g"
              % (pre_ln, fuse, n, (g[n] - g_ref[n]).abs().max().item(),
                 g_ref[n].abs().max().item(), rel(g[n], g_ref[n])))
    assert torch.allclose(y, y_ref, atol=tol, rtol=tol)
    assert torch.allclose(dx, dx_ref, atol=tol, rtol=tol)
    assert rel(dx, dx_ref) <= 2e-2
    for n in g_ref:
        assert torch.allclose(g[n], g_ref[n], atol=tol, rtol=tol), n
        assert rel(g[n], g_ref[n]) <= 2e-2, n
