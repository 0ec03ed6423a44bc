"""LLaMA model family: pre-norm blocks of RMSNorm, rotary position
embeddings on q and k, causal flash attention and a gated SiLU (SwiGLU)
feed-forward, all bias-free, with token embeddings only and an untied
head.

Hot ops ride the hand-written CDNA4 kernels: FusedRMSNorm (the residual
add before the second norm fused in), the in-place RoPE + packed-qkv flash
attention Function (q and k are rotated inside the projection's output
buffer; no unbind, no copy), and FusedSwiGLU on the packed gate/up GEMM
output.  Shapes the kernels do not take (fp32, CPU, head_dim other than
64 / 128) run apply_rope + flash_attention and the torch compositions.

Grouped-query attention (``kv_heads`` in a config, ``num_kv_heads`` on the
modules): one packed projection of H query, Hkv key and Hkv value heads;
the GQA flash kernels read K / V once per group and sum dK / dV over the
group in registers (docs/kernels.md), nothing is expanded.

Packed documents and sliding windows: ``LlamaCore.forward(ids,
segment_ids)`` keeps every token's attention inside its own document (a
maximal run of equal consecutive ids in a row), and a config's ``window``
(``mistral-7b``) limits it to the last ``window`` keys; both run the banded
causal flash kernels (ops/attention.py).  RoPE positions keep counting
along the row and do not restart per document.  The per-row bounds are
computed once per forward in LlamaCore and shared by all layers.

Out of scope: tensor-parallel sharding of the packed qkv and gate/up
weights, KV-cache decoding, and a bench.py config.
"""

import torch.nn as nn

import easyparallellibrary_amd as epl
from easyparallellibrary_amd.models.bert import StagedModel, _Stage
from easyparallellibrary_amd.models.gpt2 import synthetic_lm_batch  # noqa: F401
from easyparallellibrary_amd.models.transformer import init_weights
from easyparallellibrary_amd.ops.rms_norm import FusedRMSNorm
from easyparallellibrary_amd.ops.swiglu import FusedSwiGLU

LLAMA_CONFIGS = {
    "llama-tiny": dict(layers=2, hidden=128, heads=2, ffn=352),
    "llama-1b": dict(layers=16, hidden=2048, heads=16, ffn=5632),
    # Llama-2-7B exactly (MHA)
    "llama-7b": dict(layers=32, hidden=4096, heads=32, ffn=11008),
    "llama-tiny-gqa": dict(layers=2, hidden=128, heads=2, kv_heads=1,
                           ffn=352),
    # Llama-3-8B (GQA, 4 query heads per kv head); callers pass
    # rope_theta=500000.0 and vocab_size=128256
    "llama3-8b": dict(layers=32, hidden=4096, heads=32, kv_heads=8,
                      ffn=14336),
    # Mistral-7B: GQA with a 4096-key sliding window
    "mistral-7b": dict(layers=32, hidden=4096, heads=32, kv_heads=8,
                       ffn=14336, window=4096),
    "llama-tiny-swa": dict(layers=2, hidden=128, heads=2, kv_heads=1,
                           ffn=352, window=48),
}


class LlamaAttention(nn.Module):
    """Causal self-attention with rotary q / k; bias-free projections.
    ``num_kv_heads`` < ``num_heads`` is grouped-query attention: the one
    packed projection emits H query, Hkv key and Hkv value heads, and
    query head h attends kv head h // (H // Hkv).  ``window``: sliding
    -window attention over the last ``window`` keys."""

    def __init__(self, hidden, num_heads, num_kv_heads=None,
                 rope_theta=10000.0, window=None):
        super().__init__()
        assert hidden % num_heads == 0
        self.num_heads = num_heads
        self.num_kv_heads = num_heads if num_kv_heads is None \
            else num_kv_heads
        assert num_heads % self.num_kv_heads == 0
        self.head_dim = hidden // num_heads
        self.rope_theta = rope_theta
        self.window = window
        self.qkv = nn.Linear(
            hidden, (num_heads + 2 * self.num_kv_heads) * self.head_dim,
            bias=False)
        self.proj = nn.Linear(hidden, hidden, bias=False)

    def forward(self, x, segment_ids=None, bounds=None):
        """bounds: the band_bounds of (segment_ids, self.window) where the
        caller has computed them already (LlamaCore does, once for all
        layers)"""
        from easyparallellibrary_amd.ops.attention import (
            band_bounds, flash_attention)
        from easyparallellibrary_amd.ops.rope import (
            apply_rope, rope_qkv_flash_attention, rope_qkv_native_ok)
        b, s, h = x.shape
        if bounds is None and not (segment_ids is None
                                   and self.window is None):
            bounds = band_bounds(segment_ids, self.window, s, x.device)
        qkv = self.qkv(x)
        hq, hkv = self.num_heads, self.num_kv_heads
        if rope_qkv_native_ok(qkv, hq, hkv):
            # q and k rotated in place in the projection's own output,
            # the attention kernels read its strided slices
            o = rope_qkv_flash_attention(qkv, causal=True,
                                         theta=self.rope_theta,
                                         num_heads=hq, num_kv_heads=hkv,
                                         bounds=bounds)
        else:
            q, k, v = (t.transpose(1, 2) for t in qkv.reshape(
                b, s, hq + 2 * hkv, self.head_dim).split(
                    [hq, hkv, hkv], dim=2))
            q = apply_rope(q, theta=self.rope_theta)
            k = apply_rope(k, theta=self.rope_theta)
            o = flash_attention(q, k, v, causal=True, bounds=bounds)
        return self.proj(o.transpose(1, 2).reshape(b, s, h))


class LlamaBlock(nn.Module):
    def __init__(self, hidden, num_heads, ffn_hidden, rope_theta=10000.0,
                 eps=1e-5, num_kv_heads=None, window=None):
        super().__init__()
        self.rms1 = FusedRMSNorm(hidden, eps=eps)
        self.attn = LlamaAttention(hidden, num_heads, num_kv_heads,
                                   rope_theta=rope_theta, window=window)
        self.rms2 = FusedRMSNorm(hidden, eps=eps)
        # gate and up projections as ONE GEMM: columns [0, F) gate, [F, 2F) up
        self.fc12 = nn.Linear(hidden, 2 * ffn_hidden, bias=False)
        self.act = FusedSwiGLU()
        self.fc2 = nn.Linear(ffn_hidden, hidden, bias=False)

    def forward(self, x, segment_ids=None, bounds=None):
        a = self.attn(self.rms1(x), segment_ids, bounds)
        # residual add fused into rms2; the summed stream s is the
        # residual carried forward
        y, s = self.rms2.forward_with_sum(a, x)
        return s + self.fc2(self.act(self.fc12(y)))


class LlamaEmbedding(nn.Module):
    """Token embedding only: positions enter through RoPE."""

    def __init__(self, vocab_size, hidden):
        super().__init__()
        self.tok = nn.Embedding(vocab_size, hidden)
        nn.init.normal_(self.tok.weight, std=0.02)

    def forward(self, ids):
        return self.tok(ids)


class LlamaHead(nn.Module):
    """Final RMSNorm and the untied, bias-free projection to the vocab."""

    def __init__(self, hidden, vocab_size, eps=1e-5):
        super().__init__()
        self.norm = FusedRMSNorm(hidden, eps=eps)
        self.proj = nn.Linear(hidden, vocab_size, bias=False)

    def forward(self, x):
        return self.proj(self.norm(x))


class LlamaCore(nn.Module):
    def __init__(self, layers, hidden, heads, ffn, vocab_size,
                 rope_theta=10000.0, kv_heads=None, window=None):
        super().__init__()
        self.window = window
        self.embeddings = LlamaEmbedding(vocab_size, hidden)
        self.blocks = nn.ModuleList(
            LlamaBlock(hidden, heads, ffn, rope_theta=rope_theta,
                       num_kv_heads=kv_heads, window=window)
            for _ in range(layers))
        self.head = LlamaHead(hidden, vocab_size)

    def forward(self, ids, segment_ids=None):
        from easyparallellibrary_amd.ops.attention import band_bounds
        x = self.embeddings(ids)
        bounds = None
        if segment_ids is not None or self.window is not None:
            # once per forward, shared by every layer
            bounds = band_bounds(segment_ids, self.window, ids.shape[1],
                                 x.device)
        for b in self.blocks:
            x = b(x, segment_ids, bounds)
        return self.head(x)


class _StagedLlama(StagedModel):
    """The pipeline stages pass one tensor along: a config's ``window``
    works (a module attribute), ``segment_ids`` does not."""

    def forward(self, ids, segment_ids=None):
        if segment_ids is not None:
            raise NotImplementedError(
                "segment_ids with num_stages > 1: the staged model threads "
                "one tensor through its stages")
        return super().forward(ids)


def build_llama(config="llama-7b", vocab_size=32000, max_pos=2048,
                num_stages=1, rope_theta=10000.0):
    """Build a LLaMA under epl annotations, staged like build_gpt2.
    There are no learned positions: max_pos is only recorded on the model
    (``model.max_pos``); the RoPE tables are built on first use for the
    sequence length they meet."""
    cfg = LLAMA_CONFIGS[config] if isinstance(config, str) else dict(config)
    L, H, A, F = cfg["layers"], cfg["hidden"], cfg["heads"], cfg["ffn"]
    KV = cfg.get("kv_heads")
    W = cfg.get("window")
    if num_stages <= 1:
        with epl.replicate(device_count=1, name="stage_0"):
            model = LlamaCore(L, H, A, F, vocab_size, rope_theta=rope_theta,
                              kv_heads=KV, window=W)
        model.max_pos = max_pos
        return init_weights(model)
    per = (L + num_stages - 1) // num_stages
    stages = []
    layer_idx = 0
    for s in range(num_stages):
        with epl.replicate(device_count=1, name="stage_{}".format(s)):
            mods = []
            if s == 0:
                mods.append(LlamaEmbedding(vocab_size, H))
            n = min(per, L - layer_idx)
            mods.extend(LlamaBlock(H, A, F, rope_theta=rope_theta,
                                   num_kv_heads=KV, window=W)
                        for _ in range(n))
            layer_idx += n
            if s == num_stages - 1:
                mods.append(LlamaHead(H, vocab_size))
            stages.append(_Stage(mods))
    model = _StagedLlama(stages)
    model.max_pos = max_pos
    return init_weights(model)
