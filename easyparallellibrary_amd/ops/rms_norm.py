"""Fused RMSNorm with optional fused residual add (CDNA4 kernel, fp32
statistics) — the LLaMA counterpart of ops/layer_norm.py.

    s = x (+ residual);  rstd = rsqrt(mean(s^2) + eps);  out = s * rstd * gamma

computed in fp32 with ONE rounding at the end.  (The Hugging Face LLaMA
module rounds s * rstd to the activation dtype before the weight multiply;
this one does not, so the two differ by that one bf16 rounding.)

The HIP kernels (csrc/kernels/llama_ops.hip: rms_norm_fwd/bwd) take bf16
rows whose width is a multiple of 8 up to 8192; with a residual the add is
folded into the same pass and the summed stream s is written out (pre-norm
blocks carry it forward).  The backward folds in the gradient arriving
through the summed stream (dx += ds before the single rounding) and reduces
dgamma through per-wave partial rows in a fixed order — no atomics, so two
runs agree bitwise.  Every other input (fp32, other widths, CPU) runs the
identical math in torch.
"""

import torch
import torch.nn as nn

from easyparallellibrary_amd.ops.dispatch import native_ext, use_native

RMS_MAX_COLS = 8192


def _native_ok(x):
    return (use_native(x) and x.dtype == torch.bfloat16
            and x.shape[-1] % 8 == 0 and 8 <= x.shape[-1] <= RMS_MAX_COLS
            and x.numel() > 0)


def _aligned(*tensors):
    return all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


class _FusedRMSNorm(torch.autograd.Function):
    """y = RMSNorm(x (+ residual)).  When residual is given, also returns
    the sum s = x + residual (the pre-norm residual stream)."""

    @staticmethod
    def forward(ctx, x, residual, gamma, eps):
        x = x.contiguous()
        cols = x.shape[-1]
        rows = x.numel() // cols
        has_res = residual is not None
        if has_res:
            residual = residual.contiguous().to(x.dtype)
        ctx.param_dtype = gamma.dtype
        gamma = gamma.contiguous().to(x.dtype)
        ctx.native = _native_ok(x) and _aligned(x, residual, gamma)
        if ctx.native:
            rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
            out = torch.empty_like(x)
            s = torch.empty_like(x) if has_res else None
            native_ext().rms_norm_fwd(out, x, residual, s, gamma, rstd, eps)
            norm_in = s if has_res else x
        else:
            sf = x.float() if not has_res else x.float() + residual.float()
            sf = sf.reshape(rows, cols)
            rstd = ((sf * sf).mean(dim=1) + eps).rsqrt()
            out = (sf * rstd[:, None] * gamma.float()).to(x.dtype)
            out = out.reshape(x.shape)
            s = sf.to(x.dtype).reshape(x.shape) if has_res else None
            norm_in = s if has_res else x
        ctx.save_for_backward(norm_in, gamma, rstd)
        ctx.has_res = has_res
        # an unused output (dropping s) must not cost a zero fill and an
        # add of zeros in backward
        ctx.set_materialize_grads(False)
        if has_res:
            return out, s
        return out

    @staticmethod
    def backward(ctx, dy, *rest):
        norm_in, gamma, rstd = ctx.saved_tensors
        # with residual, grad also flows through the returned sum s
        ds = rest[0] if (ctx.has_res and rest) else None
        cols = norm_in.shape[-1]
        rows = norm_in.numel() // cols
        dgamma = None
        if dy is None:
            # only the summed stream was used: the norm contributes nothing
            dx = ds
        elif ctx.native:
            dy = dy.contiguous()
            if ds is not None:
                ds = ds.contiguous().to(norm_in.dtype)
            if not _aligned(dy, ds):
                dy = dy.clone()
                ds = ds.clone() if ds is not None else None
            dx = torch.empty_like(norm_in)
            dgamma = torch.empty(cols, dtype=torch.float32,
                                 device=norm_in.device)
            native_ext().rms_norm_bwd(dx, dgamma, dy, norm_in, gamma, rstd,
                                      ds)
        else:
            sf = norm_in.float().reshape(rows, cols)
            dyf = dy.float().reshape(rows, cols)
            xhat = sf * rstd[:, None]
            dyg = dyf * gamma.float()
            coef = (dyg * xhat).mean(dim=1, keepdim=True)
            dxf = (dyg - xhat * coef) * rstd[:, None]
            if ds is not None:
                # one rounding, as the kernel's in-register add
                dxf = dxf + ds.float().reshape(rows, cols)
            dx = dxf.to(norm_in.dtype).reshape(norm_in.shape)
            dgamma = (dyf * xhat).sum(dim=0)
        if dgamma is not None:
            dgamma = dgamma.to(ctx.param_dtype)
        # d(x) == d(residual) — the add distributes the gradient
        return dx, dx if ctx.has_res else None, dgamma, None


class FusedRMSNorm(nn.Module):
    def __init__(self, hidden, eps=1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden))
        self.eps = eps

    def forward(self, x, residual=None):
        """rms(x) — or, with residual, rms(x + residual) (fused).  The
        fused form returns only the normalized output; use
        forward_with_sum when the summed stream is needed (pre-norm)."""
        if residual is None:
            return _FusedRMSNorm.apply(x, None, self.weight, self.eps)
        out, _ = _FusedRMSNorm.apply(x, residual, self.weight, self.eps)
        return out

    def forward_with_sum(self, x, residual):
        """(rms(x+residual), x+residual) — pre-norm blocks keep the sum as
        the residual stream."""
        return _FusedRMSNorm.apply(x, residual, self.weight, self.eps)
