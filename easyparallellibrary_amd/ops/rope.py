"""Rotary position embeddings (CDNA4 kernel), HF-LLaMA half-split
convention: element i < D/2 of a head pairs with element i + D/2,

    angle(s, i) = (pos0 + s) * theta^(-i / (D/2))
    y1 = x1 cos - x2 sin,   y2 = x2 cos + x1 sin

The HIP kernel (csrc/kernels/llama_ops.hip: rope_kernel) rotates a strided
[B, S, N, D] bf16 view IN PLACE, D in (64, 128): the q and k slices of the
packed [B, S, 3, H, D] projection buffer as N = 2H heads (v is never
touched), or a stand-alone q / k.  Its ``inverse`` flag applies the
transposed rotation, which is the backward.  There is no on-device
trigonometry: cos / sin come from fp32 [L, D/2] tables computed in fp64 on
the host and rounded once.

The tables live in a module-level cache keyed by (device, D, theta, L) and
are built on first use.  They are deliberately NOT nn.Module buffers:
Engine moves a model with ``.to(device, dtype=bf16)``, which would round
them to bf16.  A graph-captured step warms up before capture, so the
table exists by then and a captured forward only reads it.
"""

import torch

from easyparallellibrary_amd.ops.attention import (
    _check_seqlens, _drop_params, _kernel_ok, _mask_tensor, _saved_optionals)
from easyparallellibrary_amd.ops.dispatch import native_ext, use_native

_TABLES = {}
_MIN_TABLE_LEN = 2048


def rope_tables(device, head_dim, theta=10000.0, length=_MIN_TABLE_LEN):
    """(cos, sin): fp32 [L, head_dim / 2] on ``device`` with L >= length.
    L is ``length`` rounded up to a power of two (at least 2048), so a
    growing sequence rebuilds the tables rarely."""
    device = torch.device(device)
    size = _MIN_TABLE_LEN
    while size < length:
        size *= 2
    key = (str(device), int(head_dim), float(theta), size)
    hit = _TABLES.get(key)
    if hit is None:
        half = head_dim // 2
        inv = torch.pow(torch.tensor(float(theta), dtype=torch.float64),
                        -torch.arange(half, dtype=torch.float64) / half)
        ang = torch.arange(size, dtype=torch.float64)[:, None] * inv[None, :]
        hit = (ang.cos().float().to(device).contiguous(),
               ang.sin().float().to(device).contiguous())
        _TABLES[key] = hit
    return hit


def _rope_torch(x, cos, sin):
    """x * cos + rotate_half(x) * sin over [.., S, D]; cos / sin [S, D/2]."""
    ct = torch.float32 if x.dtype in (torch.bfloat16, torch.float16) \
        else x.dtype
    half = x.shape[-1] // 2
    c = torch.cat([cos, cos], dim=-1).to(ct)
    s = torch.cat([sin, sin], dim=-1).to(ct)
    xf = x.to(ct)
    rot = torch.cat([-xf[..., half:], xf[..., :half]], dim=-1)
    return (xf * c + rot * s).to(x.dtype)


def _rope_native_ok(x):
    return (use_native(x) and x.dtype == torch.bfloat16 and x.dim() == 4
            and x.shape[-1] in (64, 128) and x.numel() > 0)


class _ApplyRope(torch.autograd.Function):
    """Out-of-place rotation of a [B, H, S, D] tensor: the kernel runs in
    place on a copy (forward) / on a copy of the gradient (backward)."""

    @staticmethod
    def forward(ctx, x, cos, sin, pos0):
        y = x.contiguous().clone() if x.is_contiguous() else x.contiguous()
        native_ext().rope_(y.transpose(1, 2), cos, sin, pos0, False)
        ctx.save_for_backward(cos, sin)
        ctx.pos0 = pos0
        return y

    @staticmethod
    def backward(ctx, dy):
        cos, sin = ctx.saved_tensors
        g = dy.contiguous().clone() if dy.is_contiguous() else \
            dy.contiguous()
        native_ext().rope_(g.transpose(1, 2), cos, sin, ctx.pos0, True)
        return g, None, None, None


def apply_rope(x, pos0=0, theta=10000.0):
    """Rotate x: [B, H, S, D] (q or k, any strides) by positions
    pos0 .. pos0 + S - 1.  Differentiable.  Native kernel for bf16 with
    D in (64, 128) on the GPU, the torch rotate_half composition
    elsewhere."""
    seq, d = x.shape[-2], x.shape[-1]
    if d % 2:
        raise ValueError("apply_rope needs an even head_dim, got %d" % d)
    cos, sin = rope_tables(x.device, d, theta, pos0 + seq)
    if _rope_native_ok(x):
        return _ApplyRope.apply(x, cos, sin, pos0)
    return _rope_torch(x, cos[pos0:pos0 + seq], sin[pos0:pos0 + seq])


class _RopeQKVFlashAttention(torch.autograd.Function):
    """RoPE + flash attention on the packed projection output
    [B, S, 3*H*D], no full-size copy in either direction.

    Forward rotates the q and k slices IN PLACE (the input is marked dirty
    and returned as the second output, as autograd's in-place rules ask)
    and runs attn_fwd on the strided views; the saved buffer is the rotated
    one, which is what attn_bwd needs.  Backward lets attn_bwd write into
    the slices of its own fresh d_qkv, rotates the dq / dk slices back in
    place and returns it."""

    @staticmethod
    def forward(ctx, qkv, heads, causal, scale, dropout_p, seqlens, cos, sin,
                pos0):
        b, s, width = qkv.shape
        d = width // (3 * heads)
        ctx.mark_dirty(qkv)
        packed = qkv.view(b, s, 3, heads, d)
        native_ext().rope_(packed[:, :, :2].view(b, s, 2 * heads, d), cos,
                           sin, pos0, False)
        q = packed[:, :, 0].transpose(1, 2)
        k = packed[:, :, 1].transpose(1, 2)
        v = packed[:, :, 2].transpose(1, 2)
        out = torch.empty(b, s, heads, d, dtype=qkv.dtype,
                          device=qkv.device).permute(0, 2, 1, 3)
        lse = torch.empty(b * heads * s, dtype=torch.float32,
                          device=qkv.device)
        thresh, inv_keep, seed = _drop_params(dropout_p)
        mask = _mask_tensor(b, heads, s, qkv.device) if thresh else None
        native_ext().attn_fwd(q, k, v, out, lse, scale, causal, mask, seed,
                              thresh, inv_keep, seqlens)
        ctx.has_mask = mask is not None
        ctx.has_seqlens = seqlens is not None
        ctx.save_for_backward(qkv, out, lse, cos, sin, *[
            t for t in (mask, seqlens) if t is not None])
        ctx.heads, ctx.causal, ctx.scale = heads, causal, scale
        ctx.inv_keep, ctx.pos0 = inv_keep, pos0
        ctx.set_materialize_grads(False)
        return out, qkv

    @staticmethod
    def backward(ctx, dout, drot):
        saved = ctx.saved_tensors  # ONE access: checkpoint unpack hooks
        qkv, out, lse, cos, sin = saved[:5]
        mask, seqlens = _saved_optionals(ctx, saved[5:])
        b, s, width = qkv.shape
        heads = ctx.heads
        d = width // (3 * heads)
        dqkv = torch.empty_like(qkv)
        dpacked = dqkv.view(b, s, 3, heads, d)
        if dout is None:
            dqkv.zero_()
        else:
            packed = qkv.view(b, s, 3, heads, d)
            q = packed[:, :, 0].transpose(1, 2)
            k = packed[:, :, 1].transpose(1, 2)
            v = packed[:, :, 2].transpose(1, 2)
            if not _kernel_ok(dout):
                dout = dout.contiguous()
            dq = dpacked[:, :, 0].transpose(1, 2)
            dk = dpacked[:, :, 1].transpose(1, 2)
            dv = dpacked[:, :, 2].transpose(1, 2)
            delta = torch.empty_like(lse)
            native_ext().attn_bwd(q, k, v, out, dout, lse, delta, dq, dk, dv,
                                  ctx.scale, ctx.causal, True, mask,
                                  ctx.inv_keep, None, seqlens)
        if drot is not None:
            # a consumer of the rotated buffer itself: its gradient is in
            # the rotated frame too, so it joins before the rotation back
            dqkv += drot
        native_ext().rope_(dpacked[:, :, :2].view(b, s, 2 * heads, d), cos,
                           sin, ctx.pos0, True)
        return dqkv, None, None, None, None, None, None, None, None


def rope_qkv_native_ok(qkv, heads):
    """shapes _RopeQKVFlashAttention takes: the contiguous bf16 [B, S,
    3*H*D] projection output (or its [B, S, 3, H, D] view) with
    D in (64, 128)"""
    if qkv.dim() == 5:
        if qkv.shape[2] != 3 or qkv.shape[3] != heads:
            return False
    elif qkv.dim() != 3 or qkv.shape[-1] % (3 * heads):
        return False
    d = qkv.shape[-1] if qkv.dim() == 5 else qkv.shape[-1] // (3 * heads)
    return (use_native(qkv) and qkv.dtype == torch.bfloat16
            and d in (64, 128) and qkv.is_contiguous() and qkv.numel() > 0
            and qkv.data_ptr() % 16 == 0)


def rope_qkv_flash_attention(qkv, causal=True, dropout_p=0.0, seqlens=None,
                             pos0=0, theta=10000.0, scale=None,
                             num_heads=None):
    """Rotary embedding of q and k, then flash attention, on the packed
    projection output.  Native kernels only (rope_qkv_native_ok); callers
    use apply_rope + flash_attention otherwise.

    qkv: the Linear(h, 3h) output itself, [B, S, 3*H*D] with ``num_heads``
    given — the zero-copy form: q and k are rotated in place inside the
    Linear's output buffer — or a [B, S, 3, H, D] tensor.  A 5-D tensor
    (the usual ``reshape`` of the Linear output is a VIEW of it), any other
    view, and a leaf that requires grad are cloned first: autograd routes
    an in-place change of a view through the view's base with a full-size
    copy in backward, and forbids one on such a leaf, so the copy is made
    once, in the forward only.  The kernel stays in place either way.

    Returns the attention output as a [B, H, S, D] view whose memory order
    is [B, S, H, D].  dropout_p, seqlens: as qkv_flash_attention.  pos0:
    position of the first token."""
    if qkv.dim() == 5:
        b, s, _, heads, d = qkv.shape
        if num_heads is not None and num_heads != heads:
            raise ValueError("num_heads does not match qkv")
        # the 3-D form of a 5-D tensor is a view of it: always the copy
        flat = qkv.reshape(b, s, 3 * heads * d).clone()
    else:
        if num_heads is None:
            raise ValueError("a [B, S, 3*H*D] qkv needs num_heads")
        b, s, width = qkv.shape
        heads, d = num_heads, width // (3 * num_heads)
        flat = qkv
        if flat._is_view() or (flat.is_leaf and flat.requires_grad):
            flat = flat.clone()
    if not rope_qkv_native_ok(flat, heads):
        raise ValueError(
            "rope_qkv_flash_attention needs the native kernels: contiguous "
            "bf16 qkv on the GPU with head_dim 64 or 128")
    if scale is None:
        scale = d ** -0.5
    seqlens = _check_seqlens(seqlens, flat)
    cos, sin = rope_tables(flat.device, d, theta, pos0 + s)
    out, _ = _RopeQKVFlashAttention.apply(flat, heads, causal, scale,
                                          dropout_p, seqlens, cos, sin, pos0)
    return out
