"""Hidden dropout inside the LayerNorm kernels (csrc/kernels/ln_dropout.hip)
and dropout_add, through FusedLayerNorm / dropout_add, against fp64.

The mask oracle runs no philox: x has |x| >= 0.5 everywhere, one forward
under torch.manual_seed(SEED) with a zero residual returns s = D(x), and
keep = (s != 0).  Every checked call runs under the same manual_seed, so it
draws the same kernel seed and has to use that mask whatever its residual,
entry point or kernel.

Bounds are the ones of test_layer_norm_fp64_gpu.py (kernel_refs: 2 E on
bf16 tensors, E on fp32 ones), taken at the exact D(x) = keep ? x * ik : 0
with ik the fp32 inv_keep: the forward forms s32 = fma(x, ik, res), one
rounding of the exact sum, which is the model of ln_fwd_bounds.  d_x =
bf16(fl32(g * ik)) is held to ik * E_dx (the scaled gradient's bound; the
extra fp32 rounding, 2^-24 relative, sits far inside the factor 2 on a
2^-9 bound) and the bias gradient, a sum over a subset of ik * g, to
ik * E_colsum.  dy + dy2 is exact in fp32 for the inputs used (both of
magnitude in [0.5, 8)), as ln_bwd_bounds assumes of dy.
"""

import math

import pytest
import torch

from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF = torch.bfloat16
ROWS, SEED = 5, 1234
FWD_COLS = (64, 1000, 1024, 2056, 4096)
BWD_COLS = (64, 1000, 1024, 2048)
FACTOR = kr.LN_FACTOR_BF16


def away(t):
    """|t| >= 0.5, as bf16 on the device"""
    return torch.where(t >= 0, t + 0.5, t - 0.5).to(BF).cuda()


def case(cols, rows=ROWS):
    """(module with fp32 parameters holding bf16 values, inputs)"""
    from easyparallellibrary_amd.ops.layer_norm import FusedLayerNorm
    g = torch.Generator().manual_seed(cols)
    t = {k: away(torch.randn(rows, cols, generator=g))
         for k in ("x", "res", "dy", "dy2", "ds")}
    ln = FusedLayerNorm(cols).cuda().train()
    with torch.no_grad():
        ln.weight.copy_((1 + 0.5 * torch.randn(cols, generator=g)).to(BF))
        ln.bias.copy_(torch.randn(cols, generator=g).to(BF))
    return ln, t


def inv_keep32(p):
    from easyparallellibrary_amd.ops.attention import _drop_params
    thresh, inv_keep, _ = _drop_params(p)
    return thresh, float(torch.tensor(inv_keep, dtype=torch.float32))


def oracle(ln, x, p, seed=SEED):
    torch.manual_seed(seed)
    with torch.no_grad():
        _, s = ln.forward_with_sum(x, torch.zeros_like(x), dropout_p=p)
    return (s != 0).cpu()


def dropped(x, keep, ik):
    return torch.where(keep, x.cpu().to(F64) * ik, torch.zeros((), dtype=F64))


def close(got, want, bound, factor, what):
    r = kr.ratio_of(got.detach().cpu().to(F64), want, bound)
    assert r <= factor, "%s: err/E %.3g > %g" % (what, r, factor)


@pytest.mark.parametrize("with_res", (False, True))
@pytest.mark.parametrize("p", (0.1, 0.5))
@pytest.mark.parametrize("cols", FWD_COLS)
def test_forward_fp64(cols, p, with_res):
    ln, t = case(cols)
    _, ik = inv_keep32(p)
    keep = oracle(ln, t["x"], p)
    torch.manual_seed(SEED)
    if with_res:
        y, s = ln.forward_with_sum(t["x"], t["res"], dropout_p=p)
    else:
        y = ln(t["x"], dropout_p=p)
        s = y.grad_fn.saved_tensors[0]
        assert torch.equal((s != 0).cpu(), keep)
    xd = dropped(t["x"], keep, ik)
    res = t["res"].cpu().to(F64) if with_res else None
    gamma = ln.weight.detach().cpu().to(F64)
    beta = ln.bias.detach().cpu().to(F64)
    ref = kr.ln_ref(xd, res, gamma, beta, ln.eps)
    e = kr.ln_fwd_bounds(ref, xd, res, gamma, beta, True, ln.eps)
    close(y, ref["out"], e["out"], FACTOR["out"], "y")
    close(s, ref["s"], e["s"], FACTOR["s"], "s")


@pytest.mark.parametrize("mode,with_res", (("plain", False), ("plain", True),
                                           ("dy2", False), ("dy2", True),
                                           ("dadd", True)))
@pytest.mark.parametrize("p", (0.1, 0.5))
@pytest.mark.parametrize("cols", BWD_COLS)
def test_backward_fp64(cols, p, mode, with_res):
    ln, t = case(cols)
    _, ik = inv_keep32(p)
    keep = oracle(ln, t["x"], p)
    x = t["x"].clone().requires_grad_()
    res = t["res"].clone().requires_grad_() if with_res else None
    lb = torch.zeros(cols, device="cuda", requires_grad=True)
    torch.manual_seed(SEED)
    dy, dadd = t["dy"].cpu().to(F64), None
    if mode == "dy2":
        y, y2 = ln.forward_pair(x, residual=res, lin_bias=lb, dropout_p=p)
        loss = (y * t["dy"]).sum() + (y2 * t["dy2"]).sum()
        dy = dy + t["dy2"].cpu().to(F64)
    elif mode == "dadd":
        y, s = ln.forward_with_sum(x, res, lin_bias=lb, dropout_p=p)
        loss = (y * t["dy"]).sum() + (s * t["ds"]).sum()
        dadd = t["ds"].cpu().to(F64)
    else:
        y = ln(x, residual=res, lin_bias=lb, dropout_p=p)
        loss = (y * t["dy"]).sum()
    s_used, _, mean, rstd = (v.detach().cpu().to(F64) for v in
                             y.grad_fn.saved_tensors[:4])
    wrt = [x, ln.weight, ln.bias, lb] + ([res] if with_res else [])
    grads = torch.autograd.grad(loss, wrt)
    gamma = ln.weight.detach().cpu().to(F64)
    r = kr.ln_bwd_ref(dy, s_used, gamma, mean, rstd, dadd)
    e = kr.ln_bwd_bounds(r, dy, s_used, gamma, mean, rstd, dadd, True)
    d_x_ref = torch.where(keep, r["dx"] * ik, torch.zeros((), dtype=F64))
    close(grads[0], d_x_ref, ik * e["dx"], FACTOR["dx"], "d_x")
    assert bool((grads[0].cpu()[~keep] == 0).all())
    close(grads[1], r["dgamma"], e["dgamma"], FACTOR["dgamma"], "dgamma")
    close(grads[2], r["dbeta"], e["dbeta"], FACTOR["dbeta"], "dbeta")
    close(grads[3], d_x_ref.sum(dim=0), ik * e["colsum"], FACTOR["colsum"],
          "lin_bias grad")
    if with_res:
        # the undropped gradient, everywhere; and a tensor of its own
        close(grads[4], r["dx"], e["dx"], FACTOR["dx"], "d_res")
        assert grads[4].data_ptr() != grads[0].data_ptr()


@pytest.mark.parametrize("with_res", (False, True))
@pytest.mark.parametrize("p", (0.1, 0.5))
@pytest.mark.parametrize("cols", (64, 1000, 2056))
def test_dropout_add_fp64(cols, p, with_res):
    """out = bf16(fma(x, ik, res)) and dx = bf16(fl32(g ik)): one fp32 and
    one bf16 rounding of the exact value, (v + u (1 + v)) |exact| with
    u = 2^-24 and v = 2^-8, the unit roundoff of bf16's 8 significant bits
    (2 V_BF16: kernel_refs' V_BF16 is the half of it that its factor 2 on
    bf16 tensors restores)"""
    from easyparallellibrary_amd.ops.layer_norm import dropout_add
    ln, t = case(cols)
    _, ik = inv_keep32(p)
    torch.manual_seed(SEED)
    keep = (dropout_add(t["x"], torch.zeros_like(t["x"]), p) != 0).cpu()
    assert torch.equal(keep, oracle(ln, t["x"], p))   # the LN kernels' mask
    x = t["x"].clone().requires_grad_()
    res = t["res"].clone().requires_grad_() if with_res else None
    torch.manual_seed(SEED)
    out = dropout_add(x, res, p)
    grads = torch.autograd.grad(out, [x] + ([res] if with_res else []),
                                t["dy"])
    v = 2 * kr.V_BF16
    rel = v + kr.U_F32 * (1 + v)
    want = dropped(t["x"], keep, ik)
    if with_res:
        want = want + t["res"].cpu().to(F64)
        assert torch.equal(grads[1], t["dy"])
    close(out, want, rel * want.abs(), 1.0, "out")
    dx = dropped(t["dy"], keep, ik)
    close(grads[0], dx, rel * dx.abs(), 1.0, "dx")
    assert bool((grads[0].cpu()[~keep] == 0).all())


def test_rate_and_independence():
    rows, cols, p = 4096, 1024, 0.1
    ln, t = case(cols, rows)
    thresh, _ = inv_keep32(p)
    keep = oracle(ln, t["x"], p)
    q, n = thresh / 256.0, rows * cols
    sigma = math.sqrt(q * (1 - q) / n)
    assert abs(float((~keep).double().mean()) - q) <= 5 * sigma
    assert not torch.equal(keep, oracle(ln, t["x"], p, SEED + 1))
    assert not torch.equal(keep[0], keep[1])

    def run():
        x = t["x"].clone().requires_grad_()
        res = t["res"].clone().requires_grad_()
        lb = torch.zeros(cols, device="cuda", requires_grad=True)
        torch.manual_seed(SEED)
        y = ln(x, residual=res, lin_bias=lb, dropout_p=p)
        return (y,) + torch.autograd.grad(
            y, [x, res, ln.weight, ln.bias, lb], t["dy"])

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("off", ("p0", "eval"))
def test_off_is_off(off):
    ln, t = case(1024)
    kw = {"dropout_p": 0.0}
    if off == "eval":
        ln.eval()
        kw = {"dropout_p": 0.5}

    def run(**kwargs):
        x = t["x"].clone().requires_grad_()
        res = t["res"].clone().requires_grad_()
        y, s = ln.forward_with_sum(x, res, **kwargs)
        return (y, s) + torch.autograd.grad(
            (y * t["dy"]).sum() + (s * t["ds"]).sum(),
            [x, res, ln.weight, ln.bias])

    for a, b in zip(run(), run(**kw)):
        assert torch.equal(a, b)
