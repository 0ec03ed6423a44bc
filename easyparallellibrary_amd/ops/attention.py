"""Fused flash attention (hand-written CDNA4 kernels, head_dim 64/128, bf16).

No reference counterpart (the reference's attention is plain TF ops);
this is MI355X-native hot-path work — design notes in docs/kernels.md.

Replaces torch SDPA (AOTriton) on the transformer hot path.  The HIP
kernels (csrc/kernels/attention.hip) keep the whole online softmax in
registers — swapped QK^T so each lane owns one query row, O accumulated
transposed so the rescale is lane-local, P fragments rebuilt with
v_permlane32_swap.  CPU / unsupported shapes fall back to torch SDPA.

Padded batches: ``seqlens`` (int32 [B], on the device of q) gives every
sample's number of valid leading tokens; the rest is right padding.
Query i < len attends keys j < len (and j <= i when causal); rows past
the length of out and of every gradient are exact zeros, and nothing at
a valid position depends on what the padding holds.  The kernels read
and clamp the lengths themselves (no host sync), skip the padded tiles
and exit whole blocks past the length.

Grouped-query attention: ``flash_attention`` takes k and v with Hkv heads
where Hkv divides the H heads of q; query head h attends kv head
h // (H // Hkv), the ``repeat_interleave`` order.  The GQA kernels read
K / V where they are and sum dk / dv over a group's heads in registers:
nothing is expanded and the gradients come back in the kv shape.  They
have no dropout: a GQA call with dropout_p > 0 (like fp32 and the CPU)
expands k and v and takes the torch path, where autograd does the sum.

Banded causal attention (packed documents, sliding windows):
``flash_attention`` and ``rope_qkv_flash_attention`` take ``segment_ids``
(int [B, S]) and ``window`` (int >= 1), causal only — with causal=False
either raises ValueError.  For sample b with len = clamp(seqlens[b], 0, S)
(len = S without seqlens), query i < len attends key j iff

    kv_lo[b, i] <= j <= i,   kv_lo[b, i] = max(seg_start[b, i], i - window + 1, 0)

A document is a maximal run of equal consecutive ids: ids need not be
sorted or unique, and nothing is checked on the host.  seg_start[b, i] is
the first index of the document that holds i, seg_end[b, i] one past its
last.  The kv-parallel backward kernels use the inverse bound
q_hi[b, j] = min(seg_end[b, j], j + window, S): key j is seen by queries
j <= i < min(q_hi[b, j], len).  Either argument may be None (no
restriction from it).  Rows >= len stay exact zeros; every valid row sees
at least itself, so no row is empty.  RoPE positions keep counting along
the row — they do NOT restart per document.  For finite inputs a
document's outputs and gradients do not depend on any other document of
the row.  The kernels (csrc/kernels/attention_band.hip) skip the tiles a
band excludes and serve any Hkv dividing H; dropout, fp32 and the CPU
take the torch path with the same semantics, its boolean mask built from
the same kv_lo.  ``band_bounds`` computes (kv_lo, q_hi) with torch ops and
no host sync; a caller with many layers computes them once and passes
``bounds=(kv_lo, q_hi)`` instead.

Interval attention (bidirectional packed documents, symmetric windows,
prefix-LM): ``interval_attention(q, k, v, bounds)`` and, on the packed
[B, S, 3, H, D] buffer, ``qkv_interval_attention(qkv, bounds)``.  bounds is
(kv_lo, kv_hi, q_lo, q_hi), four int32 contiguous [B or 1, S] tensors on
the device of q, each non-decreasing along S.  For sample b with
len = clamp(seqlens[b], 0, S), query i < len attends key j iff

    kv_lo[b, i] <= j < kv_hi[b, i],   kv_lo[b, i] <= i < kv_hi[b, i] <= len

and (q_lo, q_hi) describe the same mask from the key's side: key j is seen
by the queries q_lo[b, j] <= i < q_hi[b, j], q_lo[b, j] <= j < q_hi[b, j]
<= len.  The kernels (csrc/kernels/attention_interval.hip) clamp every
value where they read it (lower bounds to [0, i], upper to [i + 1, len]),
so hostile values give a wrong visible set, never a stray access or an
empty row; nothing is read on the host.  Rows >= len are exact zeros.
Writing the bounds, with pos = arange(S):

    causal           kv_lo = 0, kv_hi = pos + 1; q_lo = pos, q_hi = S
                     (flash_attention(causal=True) is the measured path)
    packed documents interval_bounds(segment_ids, None, S, device):
                     kv_lo = q_lo = seg_start, kv_hi = q_hi = seg_end
    window |i-j| < w interval_bounds(None, w, S, device):
                     kv_lo = q_lo = max(pos - w + 1, 0),
                     kv_hi = q_hi = min(pos + w, S)
    prefix-LM, p     kv_lo = 0, kv_hi = max(pos + 1, p);
                     q_lo = where(pos < p, 0, pos), q_hi = S

dropout_p runs in-kernel (csrc/kernels/attention_interval_drop.hip) with
the philox keying and the keep-bit tensor of the dense kernels, p quantized
to 1/256.  No dlse; fp32 and the CPU take the torch path (one warning per
reason), whose boolean mask comes from kv_lo / kv_hi.
"""

import os

import torch
import torch.nn.functional as F

from easyparallellibrary_amd.ops.dispatch import native_ext, use_native
from easyparallellibrary_amd.utils.logging import get_logger

logger = get_logger()
_warned = set()


def _warn_fallback(reason):
    """LOUD (once per reason) SDPA fallback: silent multi-backend
    dispatch on the hot path is exactly what the project brief
    disallows — if a model leaves the native kernels, say so."""
    if reason not in _warned:
        _warned.add(reason)
        logger.warning(
            "native attention unavailable (%s): falling back to torch "
            "SDPA for these shapes", reason)


def _kernel_ok(t):
    return (t.dim() == 4 and t.shape[-1] in (64, 128)
            and t.stride(-1) == 1
            and t.stride(1) % 8 == 0 and t.stride(2) % 8 == 0)


def _drop_params(dropout_p):
    """Quantize the drop probability to 1/256 (the kernel compares
    philox BYTES against an 8-bit threshold): returns (thresh, inv_keep,
    seed).  thresh 0 disables."""
    if not dropout_p:
        return 0, 1.0, 0
    thresh = min(255, max(1, int(round(float(dropout_p) * 256.0))))
    inv_keep = 256.0 / (256 - thresh)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return thresh, inv_keep, seed


def seqlens_from_mask(mask):
    """int32 [B] lengths from a [B, S] attention mask (non-zero = token).
    RIGHT padding only: the result is ``mask.sum(1)``, which describes
    the batch only when every sample's tokens come first."""
    return (mask != 0).sum(1).int()


def _check_seqlens(seqlens, q):
    if seqlens is None:
        return None
    if seqlens.dtype != torch.int32 or seqlens.dim() != 1 \
            or seqlens.shape[0] != q.shape[0]:
        raise ValueError("seqlens must be int32 [B={}], got {} {}".format(
            q.shape[0], seqlens.dtype, tuple(seqlens.shape)))
    if seqlens.device != q.device:
        raise ValueError("seqlens must be on the device of q")
    return seqlens.contiguous()


def _mask_tensor(b, h, seq, device):
    mask_w = (seq + 31) // 32
    return torch.empty(b * h * seq * mask_w, dtype=torch.int32,
                       device=device)


def _bwd_split():
    """The ``split_dkdv`` flag of ``attn_bwd``.  Default: the combined
    dK+dV kernel (one Q/dO stream, one exp pass) wherever it exists —
    d64, non-causal, no dropout; every other call runs the split kernels
    whatever the flag says.  EPL_ATTN_BWD_SPLIT=1 asks for the split
    dV and dK kernels everywhere; both give the same bits."""
    return os.environ.get("EPL_ATTN_BWD_SPLIT", "0") == "1"


def _saved_optionals(ctx, rest):
    """(mask, seqlens) from the tail of the saved tensors"""
    rest = list(rest)
    mask = rest.pop(0) if ctx.has_mask else None
    seqlens = rest.pop(0) if ctx.has_seqlens else None
    return mask, seqlens


class _FlashAttention(torch.autograd.Function):
    """Strided-input flash attention: the kernels consume the qkv-unbind
    views directly (no contiguous() copies); the output is written in
    [B,S,H,D] memory order so the caller's transpose+reshape is free.
    dropout_p > 0 generates the philox keep-mask in-kernel (bit tensor
    republished to the backward kernels; p quantized to 1/256)."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale, dropout_p=0.0, seqlens=None):
        if not (_kernel_ok(q) and _kernel_ok(k) and _kernel_ok(v)
                and q.stride() == k.stride() == v.stride()):
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        b, h, seq, d = q.shape
        out = torch.empty(b, seq, h, d, dtype=q.dtype,
                          device=q.device).permute(0, 2, 1, 3)
        lse = torch.empty(b * h * seq, dtype=torch.float32,
                          device=q.device)
        thresh, inv_keep, seed = _drop_params(dropout_p)
        mask = _mask_tensor(b, h, seq, q.device) if thresh else None
        native_ext().attn_fwd(q, k, v, out, lse, scale, causal, mask,
                              seed, thresh, inv_keep, seqlens)
        # optional tensors ride save_for_backward (checkpoint unpack
        # hooks see them); the flags say which ones are there
        ctx.has_mask = mask is not None
        ctx.has_seqlens = seqlens is not None
        ctx.save_for_backward(q, k, v, out, lse, *[
            t for t in (mask, seqlens) if t is not None])
        ctx.causal = causal
        ctx.scale = scale
        ctx.inv_keep = inv_keep
        return out

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors  # ONE access: checkpoint unpack hooks
        q, k, v, out, lse = saved[:5]
        mask, seqlens = _saved_optionals(ctx, saved[5:])
        # the bwd kernels re-stage q/k/v/dout tiles every 32-row iteration;
        # strided rows (6 KB apart in the qkv views) measured +405us/call
        # vs 4 contiguization copies at ~43us each — copy for backward only
        # (forward shows no strided penalty)
        orig_q = q
        contig = os.environ.get("EPL_ATTN_BWD_CONTIG", "0") == "1"
        if contig and q.stride(2) != 64:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        if not _kernel_ok(dout) or (contig and dout.stride(2) != 64):
            dout = dout.contiguous()
        # write grads in the INPUT layout: the qkv-unbind/transpose
        # backward then stacks matching-layout chunks (fast memcpy)
        # instead of strided gathers
        def grad_like(t):
            g = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype,
                                    device=t.device)
            return g
        dq = grad_like(orig_q)
        dk = grad_like(orig_q)
        dv = grad_like(orig_q)
        delta = torch.empty_like(lse)
        native_ext().attn_bwd(q, k, v, out, dout, lse, delta, dq, dk, dv,
                              ctx.scale, ctx.causal, _bwd_split(), mask,
                              ctx.inv_keep, None, seqlens)
        return dq, dk, dv, None, None, None, None


class _FlashAttentionGQA(torch.autograd.Function):
    """Grouped-query flash attention: q [B, H, S, D], k / v [B, Hkv, S, D]
    (any kernel-ok strides, k and v sharing theirs).  dk and dv are
    allocated and written in the kv shape."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale, seqlens=None):
        if not _kernel_ok(q):
            q = q.contiguous()
        if not (_kernel_ok(k) and _kernel_ok(v)
                and k.stride() == v.stride()):
            k, v = k.contiguous(), v.contiguous()
        b, h, seq, d = q.shape
        out = torch.empty(b, seq, h, d, dtype=q.dtype,
                          device=q.device).permute(0, 2, 1, 3)
        lse = torch.empty(b * h * seq, dtype=torch.float32,
                          device=q.device)
        native_ext().attn_fwd_gqa(q, k, v, out, lse, scale, causal, seqlens)
        ctx.has_seqlens = seqlens is not None
        ctx.save_for_backward(q, k, v, out, lse, *[
            t for t in (seqlens,) if t is not None])
        ctx.causal = causal
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors  # ONE access: checkpoint unpack hooks
        q, k, v, out, lse = saved[:5]
        seqlens = saved[5] if ctx.has_seqlens else None
        if not _kernel_ok(dout):
            dout = dout.contiguous()
        dq = torch.empty_strided(q.shape, q.stride(), dtype=q.dtype,
                                 device=q.device)
        dk = torch.empty_strided(k.shape, k.stride(), dtype=k.dtype,
                                 device=k.device)
        dv = torch.empty_strided(k.shape, k.stride(), dtype=k.dtype,
                                 device=k.device)
        delta = torch.empty_like(lse)
        native_ext().attn_bwd_gqa(q, k, v, out, dout, lse, delta, dq, dk,
                                  dv, ctx.scale, ctx.causal, seqlens)
        return dq, dk, dv, None, None, None


def band_bounds(segment_ids, window, seq, device):
    """(kv_lo, q_hi) of the module docstring: int32, contiguous, [B, S], or
    [1, S] when ``segment_ids`` is None (the kernels broadcast one row over
    the batch).  torch ops only, no host sync: a captured step replays
    with whatever ids the tensor then holds."""
    pos = torch.arange(seq, device=device, dtype=torch.int32)[None, :]
    kv_lo, q_hi = torch.zeros_like(pos), torch.full_like(pos, seq)
    if segment_ids is not None:
        if segment_ids.dim() != 2 or segment_ids.shape[1] != seq \
                or segment_ids.dtype.is_floating_point:
            raise ValueError("segment_ids must be an int tensor [B, S={}], "
                             "got {} {}".format(seq, segment_ids.dtype,
                                                tuple(segment_ids.shape)))
        ids = segment_ids      # on ``device`` already: no hidden copy
        change = ids[:, 1:] != ids[:, :-1]
        edge = torch.ones_like(change[:, :1])
        # a document starts at 0 and after every change: its start is the
        # running maximum of the start positions, its end the mirror image
        starts = torch.where(torch.cat([edge, change], 1), pos, 0)
        ends = torch.where(torch.cat([change, edge], 1), pos + 1, seq)
        kv_lo = starts.cummax(1).values
        q_hi = ends.flip(1).cummin(1).values.flip(1)
    if window is not None:
        if int(window) < 1:
            raise ValueError("window must be >= 1, got {}".format(window))
        kv_lo = torch.maximum(kv_lo, (pos - (int(window) - 1)).clamp(min=0))
        q_hi = torch.minimum(q_hi, (pos + int(window)).clamp(max=seq))
    return kv_lo.int().contiguous(), q_hi.int().contiguous()


def _check_bounds(bounds, q):
    kv_lo, q_hi = bounds
    for t in (kv_lo, q_hi):
        if t.dtype != torch.int32 or t.dim() != 2 \
                or t.shape[0] not in (1, q.shape[0]) \
                or t.shape[1] != q.shape[-2] or t.shape != kv_lo.shape:
            raise ValueError("bounds must be two int32 [B or 1, S] tensors")
        if t.device != q.device:
            raise ValueError("bounds must be on the device of q")
    return kv_lo.contiguous(), q_hi.contiguous()


class _FlashAttentionBand(torch.autograd.Function):
    """Banded causal flash attention: q [B, H, S, D], k / v [B, Hkv, S, D]
    with Hkv dividing H (MHA included), any kernel-ok strides consumed in
    place; kv_lo / q_hi from band_bounds.  Gradients are written in the
    input layout, dk and dv in the kv shape."""

    @staticmethod
    def forward(ctx, q, k, v, scale, kv_lo, q_hi, seqlens=None):
        if not _kernel_ok(q):
            q = q.contiguous()
        if not (_kernel_ok(k) and _kernel_ok(v)
                and k.stride() == v.stride()):
            k, v = k.contiguous(), v.contiguous()
        b, h, seq, d = q.shape
        out = torch.empty(b, seq, h, d, dtype=q.dtype,
                          device=q.device).permute(0, 2, 1, 3)
        lse = torch.empty(b * h * seq, dtype=torch.float32,
                          device=q.device)
        native_ext().attn_fwd_band(q, k, v, out, lse, scale, kv_lo, seqlens)
        ctx.has_seqlens = seqlens is not None
        ctx.save_for_backward(q, k, v, out, lse, kv_lo, q_hi, *[
            t for t in (seqlens,) if t is not None])
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors  # ONE access: checkpoint unpack hooks
        q, k, v, out, lse, kv_lo, q_hi = saved[:7]
        seqlens = saved[7] if ctx.has_seqlens else None
        if not _kernel_ok(dout):
            dout = dout.contiguous()
        dq = torch.empty_strided(q.shape, q.stride(), dtype=q.dtype,
                                 device=q.device)
        dk = torch.empty_strided(k.shape, k.stride(), dtype=k.dtype,
                                 device=k.device)
        dv = torch.empty_strided(k.shape, k.stride(), dtype=k.dtype,
                                 device=k.device)
        delta = torch.empty_like(lse)
        native_ext().attn_bwd_band(q, k, v, out, dout, lse, delta, dq, dk,
                                   dv, ctx.scale, kv_lo, q_hi, seqlens)
        return dq, dk, dv, None, None, None, None


def interval_bounds(segment_ids, window, seq, device):
    """(kv_lo, kv_hi, q_lo, q_hi) of the module docstring for packed
    bidirectional documents and / or a symmetric window |i - j| < window:
    int32, contiguous, [B, S], or [1, S] when ``segment_ids`` is None.
    Either argument may be None.  These masks are symmetric, so the query
    -side bounds are the key-side ones.  torch ops only, no host sync."""
    lo, hi = band_bounds(segment_ids, window, seq, device)
    # band_bounds' kv_lo is max(seg_start, i - w + 1) and its q_hi is
    # min(seg_end, j + w): the two ends of a symmetric interval
    return lo, hi, lo, hi


def _check_interval_bounds(bounds, q):
    bounds = tuple(bounds)
    if len(bounds) != 4:
        raise ValueError("bounds must be (kv_lo, kv_hi, q_lo, q_hi)")
    for t in bounds:
        if t.dtype != torch.int32 or t.dim() != 2 \
                or t.shape[0] not in (1, q.shape[0]) \
                or t.shape[1] != q.shape[-2] or t.shape != bounds[0].shape:
            raise ValueError("bounds must be four int32 [B or 1, S] tensors")
        if t.device != q.device:
            raise ValueError("bounds must be on the device of q")
    return tuple(t.contiguous() for t in bounds)


def _interval_fwd(q, k, v, scale, bounds, seqlens, dropout_p=0.0):
    """(out, lse, mask, inv_keep); mask is None without dropout"""
    b, h, seq, d = q.shape
    out = torch.empty(b, seq, h, d, dtype=q.dtype,
                      device=q.device).permute(0, 2, 1, 3)
    lse = torch.empty(b * h * seq, dtype=torch.float32, device=q.device)
    thresh, inv_keep, seed = _drop_params(dropout_p)
    mask = _mask_tensor(b, h, seq, q.device) if thresh else None
    native_ext().attn_fwd_interval(q, k, v, out, lse, scale, bounds[0],
                                   bounds[1], seqlens, mask, seed, thresh,
                                   inv_keep)
    return out, lse, mask, inv_keep


class _FlashAttentionInterval(torch.autograd.Function):
    """Interval flash attention: q [B, H, S, D], k / v [B, Hkv, S, D] with
    Hkv dividing H (MHA included), any kernel-ok strides consumed in place;
    the four bounds of the module docstring.  Gradients are written in the
    input layout, dk and dv in the kv shape.  dropout_p > 0: the keep
    bits are drawn in the forward kernel and saved for the backward."""

    @staticmethod
    def forward(ctx, q, k, v, scale, kv_lo, kv_hi, q_lo, q_hi, seqlens=None,
                dropout_p=0.0):
        if not _kernel_ok(q):
            q = q.contiguous()
        if not (_kernel_ok(k) and _kernel_ok(v)
                and k.stride() == v.stride()):
            k, v = k.contiguous(), v.contiguous()
        out, lse, mask, ctx.inv_keep = _interval_fwd(
            q, k, v, scale, (kv_lo, kv_hi), seqlens, dropout_p)
        ctx.has_mask = mask is not None
        ctx.has_seqlens = seqlens is not None
        ctx.save_for_backward(q, k, v, out, lse, kv_lo, kv_hi, q_lo, q_hi, *[
            t for t in (mask, seqlens) if t is not None])
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors  # ONE access: checkpoint unpack hooks
        q, k, v, out, lse = saved[:5]
        mask, seqlens = _saved_optionals(ctx, saved[9:])
        if not _kernel_ok(dout):
            dout = dout.contiguous()
        dq = torch.empty_strided(q.shape, q.stride(), dtype=q.dtype,
                                 device=q.device)
        dk = torch.empty_strided(k.shape, k.stride(), dtype=k.dtype,
                                 device=k.device)
        dv = torch.empty_strided(k.shape, k.stride(), dtype=k.dtype,
                                 device=k.device)
        native_ext().attn_bwd_interval(q, k, v, out, dout, lse,
                                       torch.empty_like(lse), dq, dk, dv,
                                       ctx.scale, *saved[5:9], seqlens, mask,
                                       ctx.inv_keep)
        return dq, dk, dv, None, None, None, None, None, None, None


class _QKVFlashAttentionInterval(torch.autograd.Function):
    """_QKVFlashAttention for interval attention: reads the q / k / v views
    of the [B, S, 3, H, D] buffer and writes dq / dk / dv into the slices
    of one d_qkv."""

    @staticmethod
    def forward(ctx, qkv, scale, kv_lo, kv_hi, q_lo, q_hi, seqlens=None,
                dropout_p=0.0):
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        out, lse, mask, ctx.inv_keep = _interval_fwd(
            q, k, v, scale, (kv_lo, kv_hi), seqlens, dropout_p)
        ctx.has_mask = mask is not None
        ctx.has_seqlens = seqlens is not None
        ctx.save_for_backward(qkv, out, lse, kv_lo, kv_hi, q_lo, q_hi, *[
            t for t in (mask, seqlens) if t is not None])
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors  # ONE access: checkpoint unpack hooks
        qkv, out, lse = saved[:3]
        mask, seqlens = _saved_optionals(ctx, saved[7:])
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        if not _kernel_ok(dout):
            dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = (dqkv[:, :, i].transpose(1, 2) for i in range(3))
        native_ext().attn_bwd_interval(q, k, v, out, dout, lse,
                                       torch.empty_like(lse), dq, dk, dv,
                                       ctx.scale, *saved[3:7], seqlens, mask,
                                       ctx.inv_keep)
        return dqkv, None, None, None, None, None, None, None


class _QKVFlashAttention(torch.autograd.Function):
    """Module-level fused path: consumes the [B,S,3,H,D] qkv projection
    buffer directly.  Forward feeds the kernels the q/k/v strided views
    (no unbind copies); backward allocates ONE d_qkv buffer and the
    kernels write dq/dk/dv straight into its slices (they take arbitrary
    shared [B,H,S] stride triplets) — no stack/CatArrayBatchedCopy, no
    3x-oversized ``empty_strided`` transients."""

    @staticmethod
    def forward(ctx, qkv, causal, scale, dropout_p=0.0, seqlens=None):
        b, s, three, h, d = qkv.shape
        q = qkv[:, :, 0].transpose(1, 2)
        k = qkv[:, :, 1].transpose(1, 2)
        v = qkv[:, :, 2].transpose(1, 2)
        out = torch.empty(b, s, h, d, dtype=qkv.dtype,
                          device=qkv.device).permute(0, 2, 1, 3)
        lse = torch.empty(b * h * s, dtype=torch.float32, device=qkv.device)
        thresh, inv_keep, seed = _drop_params(dropout_p)
        mask = _mask_tensor(b, h, s, qkv.device) if thresh else None
        native_ext().attn_fwd(q, k, v, out, lse, scale, causal, mask,
                              seed, thresh, inv_keep, seqlens)
        ctx.has_mask = mask is not None
        ctx.has_seqlens = seqlens is not None
        ctx.save_for_backward(qkv, out, lse, *[
            t for t in (mask, seqlens) if t is not None])
        ctx.causal = causal
        ctx.scale = scale
        ctx.inv_keep = inv_keep
        return out

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors  # ONE access: checkpoint unpack hooks
        qkv, out, lse = saved[:3]
        mask, seqlens = _saved_optionals(ctx, saved[3:])
        q = qkv[:, :, 0].transpose(1, 2)
        k = qkv[:, :, 1].transpose(1, 2)
        v = qkv[:, :, 2].transpose(1, 2)
        if not _kernel_ok(dout):
            dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        dq = dqkv[:, :, 0].transpose(1, 2)
        dk = dqkv[:, :, 1].transpose(1, 2)
        dv = dqkv[:, :, 2].transpose(1, 2)
        delta = torch.empty_like(lse)
        native_ext().attn_bwd(q, k, v, out, dout, lse, delta, dq, dk, dv,
                              ctx.scale, ctx.causal, _bwd_split(), mask,
                              ctx.inv_keep, None, seqlens)
        return dqkv, None, None, None, None


class _FlashAttentionLse(torch.autograd.Function):
    """Flash attention that ALSO returns the per-row lse (log-sum-exp of
    the scaled scores) as a differentiable output — the building block
    of the native ring-attention path, whose block merge weights depend
    on lse.  The incoming lse gradient folds into the backward's
    per-row delta (dS = P o (dP - (D - dlse)))."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale):
        if not (_kernel_ok(q) and _kernel_ok(k) and _kernel_ok(v)
                and q.stride() == k.stride() == v.stride()):
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        b, h, seq, d = q.shape
        out = torch.empty(b, seq, h, d, dtype=q.dtype,
                          device=q.device).permute(0, 2, 1, 3)
        lse = torch.empty(b * h * seq, dtype=torch.float32,
                          device=q.device)
        native_ext().attn_fwd(q, k, v, out, lse, scale, causal, None,
                              0, 0, 1.0)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.causal = causal
        ctx.scale = scale
        return out, lse.view(b, h, seq)

    @staticmethod
    def backward(ctx, dout, dlse):
        q, k, v, out, lse = ctx.saved_tensors
        if not _kernel_ok(dout):
            dout = dout.contiguous()

        def grad_like(t):
            return torch.empty_strided(t.shape, t.stride(), dtype=t.dtype,
                                       device=t.device)
        dq, dk, dv = grad_like(q), grad_like(q), grad_like(q)
        delta = torch.empty_like(lse)
        dlse = (dlse.reshape(-1).contiguous().float()
                if dlse is not None else None)
        native_ext().attn_bwd(q, k, v, out, dout, lse, delta, dq, dk, dv,
                              ctx.scale, ctx.causal, True, None, 1.0,
                              dlse)
        return dq, dk, dv, None, None


def flash_attention_with_lse(q, k, v, causal=False, scale=None):
    """(out, lse) — lse is [B, H, S] fp32 and differentiable.  Native
    kernel on GPU bf16 d 64/128; fp32 torch fallback elsewhere (the
    CPU tests of the ring path run through it)."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    if (use_native(q) and q.dtype == torch.bfloat16
            and q.shape[-1] in (64, 128) and q.shape == k.shape):
        # the kernels assume equal q/kv lengths (the ring contract);
        # unequal blocks take the fp32 fallback below
        return _FlashAttentionLse.apply(q, k, v, causal, scale)
    s = (q.float() @ k.float().transpose(-1, -2)) * scale
    if causal:
        seq = q.shape[-2]
        maskt = torch.triu(torch.ones(seq, seq, device=q.device,
                                      dtype=torch.bool), 1)
        s = s.masked_fill(maskt, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    out = ((s - lse.unsqueeze(-1)).exp() @ v.float()).to(q.dtype)
    return out, lse


def _masked_sdpa(q, k, v, causal, scale, dropout_p, seqlens, kv_lo=None,
                 kv_hi=None):
    """The padded-batch (and banded, ``kv_lo`` [B or 1, S]; interval, with
    ``kv_hi`` too) semantics of
    the kernels in torch ops (CPU and non-native shapes): a key mask, then
    zeros on the padded query rows.  A padded row keeps its own diagonal
    key (an empty sample: key 0), so its softmax row is finite and the
    ``where`` below hands no NaN to the backward; such rows come out zero
    like any other.  The padded rows of q, k, v are replaced by zeros
    first: a masked NaN would otherwise come through the matmuls as
    0 * NaN."""
    seq = q.shape[-2]
    pos = torch.arange(seq, device=q.device)
    if seqlens is None:
        lens = torch.full((q.shape[0],), seq, device=q.device)
    else:
        lens = seqlens.clamp(0, seq)
    keys = pos[None, :] < lens.clamp(min=1)[:, None]          # [B, S]
    attn_mask = keys[:, None, None, :]
    if causal:
        attn_mask = attn_mask & (pos[None, :] <= pos[:, None])
    if kv_lo is not None:
        attn_mask = attn_mask & (pos >= kv_lo[:, None, :, None])
        if kv_hi is not None:
            attn_mask = attn_mask & (pos < kv_hi[:, None, :, None])
        attn_mask = attn_mask | (pos[None, :] == pos[:, None])
    rows = (pos[None, :] < lens[:, None])[:, None, :, None]    # [B,1,S,1]
    q, k, v = (torch.where(rows, t, torch.zeros_like(t)) for t in (q, k, v))
    out = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask,
                                         scale=scale, dropout_p=dropout_p)
    return torch.where(rows, out, torch.zeros_like(out))


def qkv_flash_attention(qkv, causal=False, scale=None, dropout_p=0.0,
                        seqlens=None):
    """qkv: [B, S, 3, H, D] (the fused projection output).  Returns
    attention output as a [B, H, S, D] view whose memory order is
    [B, S, H, D] (the caller's transpose+reshape is free).  Requires the
    native kernels (bf16, D=64); callers fall back to the split-views +
    SDPA path otherwise.  dropout_p is applied in-kernel (philox mask,
    p quantized to 1/256) — pass it only in training mode.  seqlens:
    int32 [B] valid lengths of a right-padded batch (module docstring)."""
    if scale is None:
        scale = qkv.shape[-1] ** -0.5
    seqlens = _check_seqlens(seqlens, qkv)
    return _QKVFlashAttention.apply(qkv, causal, scale, dropout_p, seqlens)


def interval_attention(q, k, v, bounds, scale=None, seqlens=None,
                       dropout_p=0.0, allow_native=True):
    """Interval attention (module docstring).  q: [B, H, S, D]; k, v:
    [B, Hkv, S, D] with Hkv dividing H; bounds: (kv_lo, kv_hi, q_lo, q_hi),
    int32 [B or 1, S], from ``interval_bounds`` or written by the caller.
    Native kernels for bf16 / D = 64 | 128 on the GPU, dropout_p in-kernel
    (training-mode callers only; p quantized to 1/256); the torch path
    elsewhere, its boolean mask built from kv_lo / kv_hi, with the
    padded-row semantics of ``seqlens``."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    seqlens = _check_seqlens(seqlens, q)
    heads, kv_heads = q.shape[1], k.shape[1]
    if v.shape[1] != kv_heads or kv_heads < 1 or heads % kv_heads:
        raise ValueError(
            "k and v must share a head count that divides q's {}, got {} "
            "and {}".format(heads, kv_heads, v.shape[1]))
    bounds = _check_interval_bounds(bounds, q)
    if allow_native and use_native(q):
        if q.dtype != torch.bfloat16 or q.shape[-1] not in (64, 128):
            _warn_fallback("dtype={} head_dim={}".format(q.dtype,
                                                         q.shape[-1]))
        else:
            return _FlashAttentionInterval.apply(q, k, v, scale, *bounds,
                                                 seqlens, dropout_p)
    if kv_heads != heads:
        # autograd sums the expanded gradients over each group
        k = k.repeat_interleave(heads // kv_heads, dim=1)
        v = v.repeat_interleave(heads // kv_heads, dim=1)
    return _masked_sdpa(q, k, v, False, scale, dropout_p, seqlens,
                        bounds[0], bounds[1])


def qkv_interval_attention(qkv, bounds, scale=None, seqlens=None,
                           dropout_p=0.0):
    """``interval_attention`` on the packed [B, S, 3, H, D] projection
    buffer, as ``qkv_flash_attention``: a [B, H, S, D] view in [B, S, H, D]
    memory order; the backward writes one d_qkv.  Requires the native
    kernels (``qkv_native_ok``).  dropout_p is applied in-kernel — pass it
    only in training mode."""
    if scale is None:
        scale = qkv.shape[-1] ** -0.5
    seqlens = _check_seqlens(seqlens, qkv)
    bounds = _check_interval_bounds(bounds, qkv[:, :, 0].transpose(1, 2))
    return _QKVFlashAttentionInterval.apply(qkv, scale, *bounds, seqlens,
                                            dropout_p)


def qkv_native_ok(qkv):
    return (use_native(qkv) and qkv.dtype == torch.bfloat16
            and qkv.dim() == 5 and qkv.shape[-1] in (64, 128)
            and qkv.is_contiguous())


def flash_attention(q, k, v, causal=False, scale=None, allow_native=True,
                    dropout_p=0.0, seqlens=None, segment_ids=None,
                    window=None, bounds=None):
    """q: [B, H, S, D]; k, v: [B, Hkv, S, D] with Hkv dividing H (grouped
    -query attention when Hkv < H, module docstring).  Native kernel when
    bf16/D=64|128 on GPU; torch SDPA otherwise.  dropout_p runs in-kernel
    on the native path (training-mode callers only; not with GQA).
    seqlens: int32 [B] valid lengths of a right-padded batch (module
    docstring); the fallback keeps the same semantics.
    segment_ids (int [B, S]) / window (int): banded causal attention over
    packed documents / a sliding window (module docstring), causal only,
    native for any Hkv without dropout.  bounds: the (kv_lo, q_hi) that
    ``band_bounds`` returns for them, computed once by the caller."""
    if scale is None:
        scale = q.shape[-1] ** -0.5
    seqlens = _check_seqlens(seqlens, q)
    heads, kv_heads = q.shape[1], k.shape[1]
    if kv_heads != heads and (v.shape[1] != kv_heads or kv_heads < 1
                              or heads % kv_heads):
        raise ValueError(
            "k and v must share a head count that divides q's {}, got {} "
            "and {}".format(heads, kv_heads, v.shape[1]))
    banded = not (segment_ids is None and window is None and bounds is None)
    if banded:
        if not causal:
            raise ValueError("segment_ids / window need causal=True: a "
                             "non-causal band is not supported here (see "
                             "interval_attention)")
        if bounds is None:
            bounds = band_bounds(segment_ids, window, q.shape[-2], q.device)
        bounds = _check_bounds(bounds, q)
    if allow_native and use_native(q):
        if q.dtype == torch.bfloat16 and q.shape[-1] in (64, 128):
            if banded:
                if not dropout_p:
                    return _FlashAttentionBand.apply(q, k, v, scale,
                                                     *bounds, seqlens)
                _warn_fallback("banded attention with dropout")
            elif kv_heads == heads:
                return _FlashAttention.apply(q, k, v, causal, scale,
                                             dropout_p, seqlens)
            elif not dropout_p:
                return _FlashAttentionGQA.apply(q, k, v, causal, scale,
                                                seqlens)
            else:
                _warn_fallback("grouped-query attention with dropout")
        else:
            _warn_fallback("dtype={} head_dim={}".format(q.dtype,
                                                         q.shape[-1]))
    if kv_heads != heads:
        # autograd sums the expanded gradients over each group
        k = k.repeat_interleave(heads // kv_heads, dim=1)
        v = v.repeat_interleave(heads // kv_heads, dim=1)
    if banded:
        return _masked_sdpa(q, k, v, causal, scale, dropout_p, seqlens,
                            bounds[0])
    if seqlens is not None:
        return _masked_sdpa(q, k, v, causal, scale, dropout_p, seqlens)
    return F.scaled_dot_product_attention(q, k, v, is_causal=causal,
                                          scale=scale, dropout_p=dropout_p)
