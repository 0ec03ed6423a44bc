"""Transformer building blocks used by the BERT / GPT-2 / MoE model
families (the reference's model zoo is external; these are the in-repo
equivalents the benchmarks run).

Hot ops ride the hand-written CDNA4 kernels: FusedLayerNorm,
FusedBiasGelu (FFN first Linear runs bias-free), and the fused-qkv flash
attention — DEFAULT for causal and non-causal, with in-kernel philox
dropout (see _NATIVE_ATTN below).
"""

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

# Hand-written attention kernels (tests/test_attention_gpu.py) are the
# DEFAULT for causal AND non-causal shapes: the round-2 split-phase
# (branch-free bulk + masked diagonal) + 64-row bwd staging + occupancy
# tuning beats AOTriton SDPA on both hot shapes — BERT b128 h16 s512
# f+b 2049 vs 2392 us, GPT-2 b16 h25 s1024 causal f+b 1364 vs 1463 us
# (profiles/r02_attention_ab.txt).
# EPL_NATIVE_ATTENTION: "auto"/"1" (default) = native; "0" = SDPA.
_NATIVE_ATTN = os.environ.get("EPL_NATIVE_ATTENTION", "auto")

from easyparallellibrary_amd.ops.bias_gelu import FusedBiasGelu
from easyparallellibrary_amd.ops.bias_linear import FusedBiasLinear
from easyparallellibrary_amd.ops.layer_norm import (FusedLayerNorm,
                                                    linear_for_ln)

# Linear bias grads via the fused colsum kernel.  The kernel wins per-op
# (vs torch's ~2.2 TB/s reduce) but the path loses end-to-end: r1 592 vs
# 612, and the r2 retune experiment (profiles/r02_fbg_retune_ab.txt)
# showed the TunableOp table already covered the custom backward's GEMM
# shapes (tuning added zero entries) yet it still measured 593 vs 643 —
# the regression is intrinsic to the custom Function's GEMM dispatch,
# so the DEFAULT stays on torch autograd.
_FBG = os.environ.get("EPL_FUSED_BIAS_GRAD", "0") == "1"
_Linear = FusedBiasLinear if _FBG else nn.Linear

# qkv unbind backward: 1 = fused slice-copy backward (below), 0 = torch
# unbind/stack (CatArrayBatchedCopy).  A/B'd on GPU; see profiles/.
_QKV_SPLIT = os.environ.get("EPL_QKV_SPLIT", "1") == "1"


class _QKVSplit(torch.autograd.Function):
    """``unbind(dim=2)`` + ``transpose(1, 2)`` whose backward assembles
    d_qkv with three strided slice copies into ONE preallocated
    [b, s, 3, nh, d] buffer, instead of torch's stack (CatArrayBatchedCopy
    over three transposed grads, ~1.7 ms/step on BERT-Large b128)."""

    @staticmethod
    def forward(ctx, qkv):
        # qkv: [b, s, 3, nh, d] -> three [b, nh, s, d] views
        q = qkv[:, :, 0].transpose(1, 2)
        k = qkv[:, :, 1].transpose(1, 2)
        v = qkv[:, :, 2].transpose(1, 2)
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        b, nh, s, d = dq.shape
        dqkv = torch.empty((b, s, 3, nh, d), dtype=dq.dtype,
                           device=dq.device)
        dqkv[:, :, 0].copy_(dq.transpose(1, 2))
        dqkv[:, :, 1].copy_(dk.transpose(1, 2))
        dqkv[:, :, 2].copy_(dv.transpose(1, 2))
        return dqkv


class SelfAttention(nn.Module):
    def __init__(self, hidden, num_heads, causal=False, dropout=0.0):
        super().__init__()
        assert hidden % num_heads == 0
        self.hidden = hidden
        self.num_heads = num_heads
        self.head_dim = hidden // num_heads
        self.causal = causal
        self.qkv = _Linear(hidden, 3 * hidden)
        self.proj = _Linear(hidden, hidden)
        self.dropout = dropout

    def forward(self, x, bias_grad_to_ln=False, seqlens=None):
        """bias_grad_to_ln: the caller feeds the result straight into a
        FusedLayerNorm and takes (out, lin_bias) — see linear_for_ln.
        seqlens: int32 [B] valid lengths of a right-padded batch (see
        ops/attention.py); the padded rows of the attention output are
        zero, so the projection returns its bias there."""
        o = self._attend(x, seqlens)
        if bias_grad_to_ln:
            return linear_for_ln(self.proj, o)
        return self.proj(o)

    def _attend(self, x, seqlens=None):
        from easyparallellibrary_amd.ops.attention import (
            flash_attention, qkv_flash_attention, qkv_native_ok)
        b, s, h = x.shape
        qkv = self.qkv(x).reshape(b, s, 3, self.num_heads, self.head_dim)
        native_here = _NATIVE_ATTN in ("1", "auto")
        p = self.dropout if self.training else 0.0
        # dense calls keep the call they always made
        lens = {} if seqlens is None else {"seqlens": seqlens}
        if native_here and qkv_native_ok(qkv):
            # fully fused: kernels read the qkv views and write d_qkv
            # slices directly — no unbind/stack copies at all; dropout
            # runs in-kernel (philox keep-mask, p quantized to 1/256)
            o = qkv_flash_attention(qkv, causal=self.causal, dropout_p=p,
                                    **lens)
            return o.transpose(1, 2).reshape(b, s, h)
        if _QKV_SPLIT:
            q, k, v = _QKVSplit.apply(qkv)
        else:
            q, k, v = qkv.unbind(dim=2)
            q = q.transpose(1, 2)
            k = k.transpose(1, 2)
            v = v.transpose(1, 2)
        o = flash_attention(q, k, v, causal=self.causal,
                            allow_native=native_here, dropout_p=p, **lens)
        return o.transpose(1, 2).reshape(b, s, h)


class MLP(nn.Module):
    """FFN with the fused bias+GeLU kernel between the two GEMMs."""

    def __init__(self, hidden, ffn_hidden):
        super().__init__()
        self.fc1 = nn.Linear(hidden, ffn_hidden, bias=False)
        self.act = FusedBiasGelu(ffn_hidden)
        self.fc2 = _Linear(ffn_hidden, hidden)

    def forward(self, x, bias_grad_to_ln=False):
        h = self.act(self.fc1(x))
        if bias_grad_to_ln:
            return linear_for_ln(self.fc2, h)
        return self.fc2(h)


class Block(nn.Module):
    """Transformer block; pre_ln=True for GPT-style, False for BERT."""

    def __init__(self, hidden, num_heads, ffn_hidden, causal=False,
                 pre_ln=False, dropout=0.0):
        super().__init__()
        self.pre_ln = pre_ln
        self.ln1 = FusedLayerNorm(hidden)
        self.attn = SelfAttention(hidden, num_heads, causal=causal,
                                  dropout=dropout)
        self.ln2 = FusedLayerNorm(hidden)
        self.mlp = MLP(hidden, ffn_hidden)

    @staticmethod
    def _into_ln(mod, cls, x, **kwargs):
        """mod(x) for a FusedLayerNorm consumer -> (out, lin_bias); a
        wrapped or replaced submodule runs as the plain call it expects
        (plus the keyword arguments that are set, e.g. seqlens)."""
        kwargs = {k: v for k, v in kwargs.items() if v is not None}
        if type(mod) is cls:
            return mod(x, bias_grad_to_ln=True, **kwargs)
        return mod(x, **kwargs), None

    def forward(self, x, seqlens=None, x_res=None, pair_out=False):
        """seqlens: int32 [B] valid lengths of a right-padded batch; only
        the attention looks at it (every other op is per token).

        x_res / pair_out (post-LN only) carry a LayerNorm output with two
        consumers across the block boundary as the two tensors of
        FusedLayerNorm.forward_pair, so the LN backward adds their
        gradients itself: ``x_res`` is the second copy of the input (the
        attention takes x, ln1's residual takes x_res; default: x twice),
        and with ``pair_out`` the block returns both copies of its output
        for the next block.  A caller that cannot pass the pair on (a
        pipeline stage boundary, a wrapped block) leaves both out: one
        tensor is used twice and autograd adds the gradients."""
        if x_res is None:
            x_res = x
        if self.pre_ln:
            if pair_out or x_res is not x:
                raise ValueError("x_res / pair_out are post-LN only")
            # residual add fused into ln2; the summed stream s is the
            # residual carried forward
            a, pb = self._into_ln(self.attn, SelfAttention, self.ln1(x),
                                  seqlens=seqlens)
            y, s = self.ln2.forward_with_sum(a, x, lin_bias=pb)
            return s + self.mlp(y)
        # post-LN: both residual adds fuse into the LN kernels, and the
        # LN backward returns the bias gradient of the Linear before it
        a, pb = self._into_ln(self.attn, SelfAttention, x, seqlens=seqlens)
        # ln1's output feeds the MLP and ln2's residual
        h, h_res = self.ln1.forward_pair(a, residual=x_res, lin_bias=pb)
        m, fb = self._into_ln(self.mlp, MLP, h)
        if pair_out:
            return self.ln2.forward_pair(m, residual=h_res, lin_bias=fb)
        return self.ln2(m, residual=h_res, lin_bias=fb)


class Embeddings(nn.Module):
    def __init__(self, vocab_size, hidden, max_positions, use_ln=True):
        super().__init__()
        self.tok = nn.Embedding(vocab_size, hidden)
        self.pos = nn.Embedding(max_positions, hidden)
        self.ln = FusedLayerNorm(hidden) if use_ln else None
        nn.init.normal_(self.tok.weight, std=0.02)
        nn.init.normal_(self.pos.weight, std=0.02)

    def forward(self, ids, pair_out=False):
        """pair_out: return the output as the two tensors of
        FusedLayerNorm.forward_pair, for a first block that takes them as
        (x, x_res)."""
        s = ids.shape[1]
        pos = torch.arange(s, device=ids.device)
        x = self.tok(ids) + self.pos(pos)[None, :, :]
        if pair_out:
            return self.ln.forward_pair(x) if self.ln is not None else (x, x)
        if self.ln is not None:
            x = self.ln(x)
        return x


class LMHead(nn.Module):
    """Projection to vocab logits (untied for simplicity)."""

    def __init__(self, hidden, vocab_size, use_ln=True):
        super().__init__()
        self.ln = FusedLayerNorm(hidden) if use_ln else None
        self.proj = nn.Linear(hidden, vocab_size, bias=False)
        nn.init.normal_(self.proj.weight, std=0.02)

    def forward(self, x):
        if self.ln is not None:
            x = self.ln(x)
        return self.proj(x)


def init_weights(model, std=0.02):
    for m in model.modules():
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, std=std)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
    return model
