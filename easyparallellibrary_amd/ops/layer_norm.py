"""Fused LayerNorm with optional fused residual add (CDNA4 kernel,
fp32 statistics).

Replaces torch's LayerNorm on the hot path (BERT/GPT blocks run it 2x per
layer).  The HIP kernel (csrc/kernels/kernels.hip: layer_norm_fwd/bwd)
streams bf16 rows as packed 16-byte loads with fp32 accumulation, stages
the fp32 row image in LDS between the statistics and normalize passes
(no HBM re-read), and — with a residual input — folds the residual add
into the same pass, eliminating the separate elementwise-add kernel
entirely (post-LN BERT: x = LN(x + sublayer(x))).  The backward caches
xhat / dy in registers, writes dgamma/dbeta as one partial row per block
that a small fixed-order kernel reduces and writes in the parameter
dtype (no zero fill, no cast, no atomics), and can fold three neighbours
in: the gradient arriving through the summed stream (dx += ds), the bias
gradient of the Linear that produced x (column sum of dx), and the add of
the gradients of an output with two consumers (dy + dy2, see
FusedLayerNorm.forward_pair).
CPU fallback = identical math in torch (numerics tests compare against a
plain fp32 torch reference).
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from easyparallellibrary_amd.ops.dispatch import native_ext, use_native


# EPL_LN_BWD_FUSE: "1" (default) = blocks hand the bias gradient of the
# Linear feeding a LayerNorm to the LN backward kernel (its column sum of
# dx) instead of a separate reduction; "0" = every Linear reduces its own
# bias gradient.  Read once; the A/B and the tests flip it.
_LN_BWD_FUSE = os.environ.get("EPL_LN_BWD_FUSE", "1") == "1"

# EPL_LN_BWD_FORK: "1" (default) = forward_pair hands a LayerNorm output
# with two consumers out as two tensors on one storage, so their gradients
# reach the LN backward separately and the kernel adds them while it
# loads; "0" = one tensor used twice, autograd adds the gradients in a
# kernel of its own.  Read once; the A/B and the tests flip it.
_LN_BWD_FORK = os.environ.get("EPL_LN_BWD_FORK", "1") == "1"


def _native_ok(x):
    return (use_native(x) and x.dtype in (torch.bfloat16, torch.float32)
            and x.shape[-1] % 8 == 0)


def _bwd_fast_ok(x):
    """Shapes the one-row-per-wave backward kernel takes — the only ones
    with the in-kernel dadd / colsum."""
    return (_native_ok(x) and x.dtype == torch.bfloat16
            and x.shape[-1] <= 2048)


def layer_norm_bwd_fused(dy, x, gamma, mean, rstd, dadd=None,
                         want_colsum=False, dy2=None, param_dtype=None,
                         colsum_dtype=None):
    """Native LN backward of ``dy (+ dy2)`` at the saved (x, mean, rstd),
    plus ``dadd`` added into dx and, if asked, colsum = dx.sum(rows).
    Fast-path shapes do all of it inside the kernel and get dgamma / dbeta
    in ``param_dtype`` and colsum in ``colsum_dtype`` (both default fp32)
    straight from the reduce kernel; the others keep the separate adds,
    sum and casts.  Returns (dx, dgamma, dbeta, colsum | None)."""
    cols = x.shape[-1]
    param_dtype = param_dtype or torch.float32
    colsum_dtype = colsum_dtype or torch.float32
    dx = torch.empty_like(x)
    if _bwd_fast_ok(x):
        typed = (torch.bfloat16, torch.float32)
        # the reduce kernel writes bf16 or fp32; anything else is cast
        pd = param_dtype if param_dtype in typed else torch.float32
        cd = colsum_dtype if colsum_dtype in typed else torch.float32
        dgamma = torch.empty(cols, dtype=pd, device=x.device)
        dbeta = torch.empty(cols, dtype=pd, device=x.device)
        colsum = (torch.empty(cols, dtype=cd, device=x.device)
                  if want_colsum else None)
        if dadd is not None:
            dadd = dadd.contiguous().to(x.dtype)
        if dy2 is not None:
            dy2 = dy2.contiguous().to(x.dtype)
        native_ext().layer_norm_bwd_typed(dx, dgamma, dbeta, dy, x, gamma,
                                          mean, rstd, dadd, colsum, dy2)
        if colsum is not None:
            colsum = colsum.to(colsum_dtype)
        return (dx, dgamma.to(param_dtype), dbeta.to(param_dtype), colsum)
    if dy2 is not None:
        dy = dy + dy2
    dgamma = torch.zeros(cols, dtype=torch.float32, device=x.device)
    dbeta = torch.zeros(cols, dtype=torch.float32, device=x.device)
    native_ext().layer_norm_bwd(dx, dgamma, dbeta, dy, x, gamma, mean, rstd)
    if dadd is not None:
        dx = dx + dadd
    colsum = (dx.reshape(-1, cols).sum(dim=0, dtype=torch.float32)
              .to(colsum_dtype) if want_colsum else None)
    return dx, dgamma.to(param_dtype), dbeta.to(param_dtype), colsum


class _FusedLayerNorm(torch.autograd.Function):
    """y = LN(x (+ residual)).  When residual is given, also returns the
    sum s = x + residual (the pre-LN residual stream).

    ``lin_bias`` (optional) is the bias parameter of the Linear that
    produced x, whose forward ran with that bias detached.  It does not
    enter the forward math; its gradient is the column sum of dx, which
    the backward kernel accumulates next to dgamma/dbeta.

    ``fork``: return y twice, as two tensors on one storage (y, y2[, s]),
    for a y with two consumers: backward then receives the two gradients
    separately and the kernel adds them in fp32 as it loads them."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps, lin_bias=None,
                fork=False):
        x = x.contiguous()
        cols = x.shape[-1]
        rows = x.numel() // cols
        has_res = residual is not None
        if has_res:
            # the kernel derives its dtype from x; autocast can hand us
            # a bf16 x with an fp32 residual stream (or vice versa)
            residual = residual.contiguous().to(x.dtype)
        ctx.param_dtype = gamma.dtype
        gamma = gamma.contiguous().to(x.dtype)
        beta = beta.contiguous().to(x.dtype)
        if _native_ok(x):
            mean = torch.empty(rows, dtype=torch.float32, device=x.device)
            rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
            out = torch.empty_like(x)
            s = torch.empty_like(x) if has_res else None
            native_ext().layer_norm_fwd(out, x, residual, s, gamma,
                                        beta, mean, rstd, eps)
            norm_in = s if has_res else x
        else:
            norm_in = (x + residual) if has_res else x
            xf = norm_in.float().reshape(rows, cols)
            mu = xf.mean(dim=1)
            var = xf.var(dim=1, unbiased=False)
            rstd = (var + eps).rsqrt()
            mean = mu
            xhat = (xf - mu[:, None]) * rstd[:, None]
            out = (xhat * gamma.float() + beta.float()).to(x.dtype)
            out = out.reshape(x.shape)
            s = norm_in if has_res else None
        ctx.save_for_backward(norm_in, gamma, mean, rstd)
        ctx.has_res = has_res
        ctx.bias_dtype = lin_bias.dtype if lin_bias is not None else None
        ctx.fuse = _LN_BWD_FUSE
        if ctx.fuse:
            # an unused output (post-LN drops s) must not cost a zero
            # fill and an add of zeros in backward
            ctx.set_materialize_grads(False)
        ctx.fork = fork
        outs = (out, out.view_as(out)) if fork else (out,)
        if has_res:
            outs = outs + (s,)
        return outs if len(outs) > 1 else out

    @staticmethod
    def backward(ctx, dy, *rest):
        norm_in, gamma, mean, rstd = ctx.saved_tensors
        dy2 = None
        if ctx.fork:
            # the second copy's gradient; an unused copy arrives as None
            dy2, rest = rest[0], rest[1:]
            if dy is None:
                dy, dy2 = dy2, None
        # with residual, grad also flows through the returned sum s
        ds = rest[0] if (ctx.has_res and rest) else None
        # switch off: the summed stream's gradient is added separately
        ds_late = None
        if not ctx.fuse:
            ds, ds_late = None, ds
        want_db = ctx.bias_dtype is not None and ctx.needs_input_grad[5]
        cols = norm_in.shape[-1]
        rows = norm_in.numel() // cols
        dgamma = dbeta = colsum = None
        if dy is None:
            # only the summed stream was used: LN contributes nothing
            dx = ds
            if dx is not None and want_db:
                colsum = dx.reshape(rows, cols).sum(dim=0,
                                                    dtype=torch.float32)
        elif _native_ok(norm_in):
            dx, dgamma, dbeta, colsum = layer_norm_bwd_fused(
                dy.contiguous(), norm_in, gamma.contiguous(), mean, rstd,
                dadd=ds, want_colsum=want_db, dy2=dy2,
                param_dtype=ctx.param_dtype, colsum_dtype=ctx.bias_dtype)
        else:
            if dy2 is not None:
                # in the compute dtype, as autograd's own add
                dy = dy + dy2
            xf = norm_in.float().reshape(rows, cols)
            dyf = dy.float().reshape(rows, cols)
            xhat = (xf - mean[:, None]) * rstd[:, None]
            dyg = dyf * gamma.float()
            c1 = dyg.mean(dim=1, keepdim=True)
            c2 = (dyg * xhat).mean(dim=1, keepdim=True)
            dxf = (dyg - c1 - xhat * c2) * rstd[:, None]
            if ds is not None:
                # one rounding, as the kernel's in-register add
                dxf = dxf + ds.float().reshape(rows, cols)
            if want_db:
                colsum = dxf.sum(dim=0)
            dx = dxf.to(norm_in.dtype).reshape(norm_in.shape)
            dgamma = (dyf * xhat).sum(dim=0)
            dbeta = dyf.sum(dim=0)
        if dgamma is not None:
            dgamma = dgamma.to(ctx.param_dtype)
            dbeta = dbeta.to(ctx.param_dtype)
        if ds_late is not None:
            dx = dx + ds_late
        dbias = colsum.to(ctx.bias_dtype) if colsum is not None else None
        # d(x) == d(residual) — the add distributes the gradient
        return (dx, dx if ctx.has_res else None, dgamma, dbeta, None, dbias,
                None)


class FusedLayerNorm(nn.Module):
    def __init__(self, hidden, eps=1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden))
        self.bias = nn.Parameter(torch.zeros(hidden))
        self.eps = eps

    def forward(self, x, residual=None, lin_bias=None):
        """ln(x) — or, with residual, ln(x + residual) (fused).  The
        fused form returns only the normalized output; use
        forward_with_sum when the summed stream is needed (pre-LN).

        lin_bias: bias parameter of the Linear that produced x, when
        that Linear ran with the bias detached (see linear_for_ln): its
        gradient then comes out of this LN's backward."""
        if residual is None:
            return _FusedLayerNorm.apply(x, None, self.weight, self.bias,
                                         self.eps, lin_bias)
        out, _ = _FusedLayerNorm.apply(x, residual, self.weight, self.bias,
                                       self.eps, lin_bias)
        return out

    def forward_pair(self, x, residual=None, lin_bias=None):
        """forward() for an output with TWO consumers: returns (y, y2),
        the same values twice.  With the fork on (EPL_LN_BWD_FORK, and
        grad mode) they are two tensors on one storage and each consumer
        takes its own, so the LN backward kernel receives both gradients
        and adds them itself; otherwise y2 is y and autograd adds."""
        if not (_LN_BWD_FORK and torch.is_grad_enabled()):
            y = self.forward(x, residual=residual, lin_bias=lin_bias)
            return y, y
        outs = _FusedLayerNorm.apply(x, residual, self.weight, self.bias,
                                     self.eps, lin_bias, True)
        return outs[0], outs[1]

    def forward_with_sum(self, x, residual, lin_bias=None):
        """(ln(x+residual), x+residual) — pre-LN blocks keep the sum as
        the residual stream."""
        return _FusedLayerNorm.apply(x, residual, self.weight, self.bias,
                                     self.eps, lin_bias)


def linear_for_ln(lin, x):
    """Run ``lin`` on x for a consumer that is a FusedLayerNorm.

    Returns (y, lin_bias).  When the LN backward can deliver the bias
    gradient (plain nn.Linear whose bias requires grad, switch on),
    the forward runs with the bias detached — same GEMM, same bias
    epilogue, same result — so autograd skips the Linear's own bias
    reduction, and lin_bias is the parameter to hand to the LN.
    Otherwise (y, None): the Linear runs as the module it is."""
    if (_LN_BWD_FUSE and type(lin) is nn.Linear and lin.bias is not None
            and lin.bias.requires_grad and torch.is_grad_enabled()):
        return F.linear(x, lin.weight, lin.bias.detach()), lin.bias
    return lin(x), None
