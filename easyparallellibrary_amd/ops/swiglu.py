"""Fused SwiGLU gate (CDNA4 kernel): out = silu(gate) * up, with gate and
up the two halves of ONE packed [.., 2F] GEMM output — gate = columns
[0, F), up = [F, 2F).

The LLaMA feed-forward runs its gate and up projections as one bias-free
Linear(h, 2F); this op replaces the chunk, the SiLU and the multiply with
one streaming pass, and its backward writes both halves of one [.., 2F]
gradient buffer, so the weight-gradient GEMM sees a single tensor (no cat).
The sigmoid is 1 / (1 + 2^(-g log2 e)) from one v_exp_f32 and one v_rcp_f32,
shared by the value and the derivative; every stored bf16 value is rounded
once (csrc/kernels/llama_ops.hip: swiglu_fwd/bwd).

Native path: bf16 with F % 8 == 0.  Everything else is the torch
composition F.silu(g) * u.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from easyparallellibrary_amd.ops.dispatch import native_ext, use_native


def _native_ok(gu):
    return (use_native(gu) and gu.dtype == torch.bfloat16
            and gu.shape[-1] % 16 == 0 and gu.numel() > 0)


class _FusedSwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        gu = gu.contiguous()
        if gu.data_ptr() % 16:
            gu = gu.clone()
        out = torch.empty(gu.shape[:-1] + (gu.shape[-1] // 2,),
                          dtype=gu.dtype, device=gu.device)
        native_ext().swiglu_fwd(out, gu)
        ctx.save_for_backward(gu)
        return out

    @staticmethod
    def backward(ctx, dy):
        gu, = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.data_ptr() % 16:
            dy = dy.clone()
        dgu = torch.empty_like(gu)
        native_ext().swiglu_bwd(dgu, dy, gu)
        return dgu


def swiglu(gu):
    """silu(gu[..., :F]) * gu[..., F:] for a packed [.., 2F] tensor."""
    if gu.shape[-1] % 2:
        raise ValueError("swiglu needs an even packed width, got {}".format(
            gu.shape[-1]))
    if _native_ok(gu):
        return _FusedSwiGLU.apply(gu)
    g, u = gu.chunk(2, dim=-1)
    return F.silu(g) * u


class FusedSwiGLU(nn.Module):
    """Activation between Linear(h, 2F) and Linear(F, h); no parameters."""

    def forward(self, gu):
        return swiglu(gu)
