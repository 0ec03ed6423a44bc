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

Hidden dropout (``dropout_p``; csrc/kernels/ln_dropout.hip) drops x before
the residual add, inside the same kernels: s = D(x) + residual,
y = LN(s), with D(x) = keep ? x / (1 - p) : 0 and p quantized to 1/256 as
for attention dropout.  keep is a philox function of (seed, row, column)
that the backward kernels evaluate again from the seed kept in ctx: no
mask tensor exists.  The backward returns TWO gradients, d_residual = g
and d_x = D(g), and the bias gradient of the Linear before is the column
sum of d_x.  bf16 rows of cols % 8 == 0 and cols <= 4096 run the kernels
(cols > 2048: the LN backward is the generic one and the drop of the
gradient a kernel of its own); every other input draws a mask with
F.dropout and keeps it for the backward.  ``dropout_add`` is the same
D(x) (+ residual) for the sites with no LayerNorm behind them.  The seed
is a scalar kernel argument drawn on the host, so a replayed hipGraph
reuses the mask of its capture.
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


def _drop_native_ok(x):
    """Shapes the dropout kernels take: the forward and dropout_add (the
    fused backward takes the _bwd_fast_ok ones among them)."""
    return (use_native(x) and x.dtype == torch.bfloat16
            and x.shape[-1] % 8 == 0 and x.numel() > 0
            and x.data_ptr() % 16 == 0)


def _drop_ln_ok(x):
    return _drop_native_ok(x) and x.shape[-1] <= 4096


def _drop_scale(p):
    return 1.0 / (1.0 - p) if p < 1.0 else 0.0


def _draw_keep(x, p):
    """bool keep mask of x's shape from torch's generator, the draw
    F.dropout(x, p) makes."""
    return F.dropout(torch.ones_like(x), p, True) != 0


def _drop(g, drop):
    """D(g) by the stand-alone kernel, with the mask of ``drop``"""
    thresh, inv_keep, seed = drop
    g = g.contiguous()
    out = torch.empty_like(g)
    native_ext().dropout_add_bwd(out, g, seed, thresh, inv_keep)
    return out


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
    separately and the kernel adds them in fp32 as it loads them.

    ``dropout_p`` > 0: x is dropped before the add (module docstring) and
    backward returns d_x and d_residual as two tensors.  ``seed``: the
    philox seed of the native path; drawn here when None."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps, lin_bias=None,
                fork=False, dropout_p=0.0, seed=None):
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
        ctx.drop = None        # (thresh, inv_keep, seed) of the kernels
        keep = None            # mask tensor of the torch path
        if dropout_p and _drop_ln_ok(x):
            from easyparallellibrary_amd.ops.attention import _drop_params
            thresh, inv_keep, drawn = _drop_params(dropout_p)
            ctx.drop = (thresh, inv_keep, drawn if seed is None else seed)
        elif dropout_p:
            keep = _draw_keep(x, dropout_p)
            ctx.scale = _drop_scale(dropout_p)
            x = torch.where(keep, x * ctx.scale, torch.zeros_like(x))
        if ctx.drop is not None:
            mean = torch.empty(rows, dtype=torch.float32, device=x.device)
            rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
            out = torch.empty_like(x)
            s = torch.empty_like(x)
            native_ext().layer_norm_dropout_fwd(
                out, x, residual, s, gamma, beta, mean, rstd, eps,
                ctx.drop[2], ctx.drop[0], ctx.drop[1])
            norm_in = s
            if not has_res:
                s = None
        elif _native_ok(x):
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
        ctx.has_keep = keep is not None
        ctx.save_for_backward(norm_in, gamma, mean, rstd,
                              *([keep] if ctx.has_keep else []))
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
        norm_in, gamma, mean, rstd = ctx.saved_tensors[:4]
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
        if ctx.drop is not None:
            return _FusedLayerNorm._drop_backward(ctx, dy, dy2, ds, ds_late,
                                                  want_db)
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
        if ctx.has_keep and dx is not None:
            # torch-path dropout: the residual takes g, x takes D(g)
            d_res = dx
            dx = torch.where(ctx.saved_tensors[4], d_res * ctx.scale,
                             torch.zeros_like(d_res))
            if want_db:
                colsum = dx.reshape(rows, cols).sum(dim=0,
                                                    dtype=torch.float32)
            dbias = colsum.to(ctx.bias_dtype) if want_db else None
            return (dx, d_res if ctx.has_res else None, dgamma, dbeta, None,
                    dbias, None, None, None)
        dbias = colsum.to(ctx.bias_dtype) if colsum is not None else None
        # d(x) == d(residual) — the add distributes the gradient
        return (dx, dx if ctx.has_res else None, dgamma, dbeta, None, dbias,
                None, None, None)

    @staticmethod
    def _drop_backward(ctx, dy, dy2, ds, ds_late, want_db):
        """backward of the native dropout forward: d_res = g, the gradient
        of s, and d_x = D(g) with the keep of ctx.drop."""
        s, gamma, mean, rstd = ctx.saved_tensors[:4]
        thresh, inv_keep, seed = ctx.drop
        cols = s.shape[-1]
        typed = (torch.bfloat16, torch.float32)
        dgamma = dbeta = colsum = None
        if dy is not None and ds_late is None and _bwd_fast_ok(s):
            # one kernel: both gradients, dgamma / dbeta and the colsum
            pd = ctx.param_dtype if ctx.param_dtype in typed \
                else torch.float32
            cd = ctx.bias_dtype if ctx.bias_dtype in typed else torch.float32
            d_x, d_res = torch.empty_like(s), torch.empty_like(s)
            dgamma = torch.empty(cols, dtype=pd, device=s.device)
            dbeta = torch.empty(cols, dtype=pd, device=s.device)
            if want_db:
                colsum = torch.empty(cols, dtype=cd, device=s.device)
            native_ext().layer_norm_dropout_bwd(
                d_x, d_res, dgamma, dbeta, dy.contiguous().to(s.dtype), s,
                gamma.contiguous(), mean, rstd,
                None if ds is None else ds.contiguous().to(s.dtype), colsum,
                None if dy2 is None else dy2.contiguous().to(s.dtype),
                seed, thresh, inv_keep)
        else:
            # wide rows, the fusion switch off, or only s was used: g by
            # the plain path, then the drop as a pass of its own
            if dy is None:
                d_res = ds
            else:
                d_res, dgamma, dbeta, _ = layer_norm_bwd_fused(
                    dy.contiguous(), s, gamma.contiguous(), mean, rstd,
                    dadd=ds, dy2=dy2, param_dtype=ctx.param_dtype)
            if ds_late is not None:
                d_res = d_res + ds_late
            d_x = None
            if d_res is not None:
                d_res = d_res.contiguous().to(s.dtype)
                d_x = _drop(d_res, ctx.drop)
                if want_db:
                    colsum = d_x.reshape(-1, cols).sum(dim=0,
                                                       dtype=torch.float32)
        if dgamma is not None:
            dgamma = dgamma.to(ctx.param_dtype)
            dbeta = dbeta.to(ctx.param_dtype)
        dbias = colsum.to(ctx.bias_dtype) if colsum is not None else None
        return (d_x, d_res if ctx.has_res else None, dgamma, dbeta, None,
                dbias, None, None, None)


class FusedLayerNorm(nn.Module):
    def __init__(self, hidden, eps=1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden))
        self.bias = nn.Parameter(torch.zeros(hidden))
        self.eps = eps

    def _run(self, x, residual, lin_bias, fork, dropout_p):
        # without dropout: the call this module always made
        if not (dropout_p and self.training):
            if fork:
                return _FusedLayerNorm.apply(x, residual, self.weight,
                                             self.bias, self.eps, lin_bias,
                                             True)
            return _FusedLayerNorm.apply(x, residual, self.weight, self.bias,
                                         self.eps, lin_bias)
        return _FusedLayerNorm.apply(x, residual, self.weight, self.bias,
                                     self.eps, lin_bias, fork,
                                     float(dropout_p))

    def forward(self, x, residual=None, lin_bias=None, dropout_p=0.0):
        """ln(x) — or, with residual, ln(x + residual) (fused).  The
        fused form returns only the normalized output; use
        forward_with_sum when the summed stream is needed (pre-LN).

        lin_bias: bias parameter of the Linear that produced x, when
        that Linear ran with the bias detached (see linear_for_ln): its
        gradient then comes out of this LN's backward.

        dropout_p (here and in forward_pair / forward_with_sum): hidden
        dropout of x before the add, ln(D(x) + residual), in training
        mode only (module docstring)."""
        if residual is None:
            return self._run(x, None, lin_bias, False, dropout_p)
        out, _ = self._run(x, residual, lin_bias, False, dropout_p)
        return out

    def forward_pair(self, x, residual=None, lin_bias=None, dropout_p=0.0):
        """forward() for an output with TWO consumers: returns (y, y2),
        the same values twice.  With the fork on (EPL_LN_BWD_FORK, and
        grad mode) they are two tensors on one storage and each consumer
        takes its own, so the LN backward kernel receives both gradients
        and adds them itself; otherwise y2 is y and autograd adds."""
        if not (_LN_BWD_FORK and torch.is_grad_enabled()):
            y = self.forward(x, residual=residual, lin_bias=lin_bias,
                             dropout_p=dropout_p)
            return y, y
        outs = self._run(x, residual, lin_bias, True, dropout_p)
        return outs[0], outs[1]

    def forward_with_sum(self, x, residual, lin_bias=None, dropout_p=0.0):
        """(ln(x+residual), x+residual) — pre-LN blocks keep the sum as
        the residual stream."""
        return self._run(x, residual, lin_bias, False, dropout_p)


class _DropoutAdd(torch.autograd.Function):
    """out = D(x) (+ residual) by the stand-alone kernels, with the keep
    of the LN dropout kernels for the same seed, rows and columns."""

    @staticmethod
    def forward(ctx, x, residual, dropout_p, seed=None):
        from easyparallellibrary_amd.ops.attention import _drop_params
        thresh, inv_keep, drawn = _drop_params(dropout_p)
        ctx.drop = (thresh, inv_keep, drawn if seed is None else seed)
        ctx.has_res = residual is not None
        x = x.contiguous()
        if ctx.has_res:
            residual = residual.contiguous().to(x.dtype)
        out = torch.empty_like(x)
        native_ext().dropout_add_fwd(out, x, residual, ctx.drop[2], thresh,
                                     inv_keep)
        return out

    @staticmethod
    def backward(ctx, g):
        return (_drop(g, ctx.drop), g if ctx.has_res else None, None, None)


def dropout_add(x, residual=None, p=0.0, training=True):
    """D(x) (+ residual): hidden dropout where no LayerNorm follows (the
    pre-LN tail s + D(mlp(y)), the embeddings).  bf16 device tensors with
    cols % 8 == 0 run the kernel; the others F.dropout and torch's add."""
    if not (p and training):
        return x if residual is None else residual + x
    if _drop_native_ok(x):
        return _DropoutAdd.apply(x, residual, float(p))
    x = F.dropout(x, p, True)
    return x if residual is None else residual + x


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
