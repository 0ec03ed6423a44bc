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

Out of scope: grouped-query attention (the attention kernels take equal
q and kv head counts; Llama-2-7B, the largest config here, is MHA), tensor
-parallel sharding of the packed gate/up weight, and a bench.py config.
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
}


class LlamaAttention(nn.Module):
    """Causal self-attention with rotary q / k; bias-free projections."""

    def __init__(self, hidden, num_heads, rope_theta=10000.0):
        super().__init__()
        assert hidden % num_heads == 0
        self.num_heads = num_heads
        self.head_dim = hidden // num_heads
        self.rope_theta = rope_theta
        self.qkv = nn.Linear(hidden, 3 * hidden, bias=False)
        self.proj = nn.Linear(hidden, hidden, bias=False)

    def forward(self, x):
        from easyparallellibrary_amd.ops.attention import flash_attention
        from easyparallellibrary_amd.ops.rope import (
            apply_rope, rope_qkv_flash_attention, rope_qkv_native_ok)
        b, s, h = x.shape
        qkv = self.qkv(x)
        if rope_qkv_native_ok(qkv, self.num_heads):
            # q and k rotated in place in the projection's own output,
            # the attention kernels read its strided slices
            o = rope_qkv_flash_attention(qkv, causal=True,
                                         theta=self.rope_theta,
                                         num_heads=self.num_heads)
        else:
            q, k, v = (t.transpose(1, 2) for t in qkv.reshape(
                b, s, 3, self.num_heads, self.head_dim).unbind(dim=2))
            q = apply_rope(q, theta=self.rope_theta)
            k = apply_rope(k, theta=self.rope_theta)
            o = flash_attention(q, k, v, causal=True)
        return self.proj(o.transpose(1, 2).reshape(b, s, h))


class LlamaBlock(nn.Module):
    def __init__(self, hidden, num_heads, ffn_hidden, rope_theta=10000.0,
                 eps=1e-5):
        super().__init__()
        self.rms1 = FusedRMSNorm(hidden, eps=eps)
        self.attn = LlamaAttention(hidden, num_heads, rope_theta=rope_theta)
        self.rms2 = FusedRMSNorm(hidden, eps=eps)
        # gate and up projections as ONE GEMM: columns [0, F) gate, [F, 2F) up
        self.fc12 = nn.Linear(hidden, 2 * ffn_hidden, bias=False)
        self.act = FusedSwiGLU()
        self.fc2 = nn.Linear(ffn_hidden, hidden, bias=False)

    def forward(self, x):
        a = self.attn(self.rms1(x))
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
                 rope_theta=10000.0):
        super().__init__()
        self.embeddings = LlamaEmbedding(vocab_size, hidden)
        self.blocks = nn.ModuleList(
            LlamaBlock(hidden, heads, ffn, rope_theta=rope_theta)
            for _ in range(layers))
        self.head = LlamaHead(hidden, vocab_size)

    def forward(self, ids):
        x = self.embeddings(ids)
        for b in self.blocks:
            x = b(x)
        return self.head(x)


def build_llama(config="llama-7b", vocab_size=32000, max_pos=2048,
                num_stages=1, rope_theta=10000.0):
    """Build a LLaMA under epl annotations, staged like build_gpt2.
    There are no learned positions: max_pos is only recorded on the model
    (``model.max_pos``); the RoPE tables are built on first use for the
    sequence length they meet."""
    cfg = LLAMA_CONFIGS[config] if isinstance(config, str) else dict(config)
    L, H, A, F = cfg["layers"], cfg["hidden"], cfg["heads"], cfg["ffn"]
    if num_stages <= 1:
        with epl.replicate(device_count=1, name="stage_0"):
            model = LlamaCore(L, H, A, F, vocab_size, rope_theta=rope_theta)
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
            mods.extend(LlamaBlock(H, A, F, rope_theta=rope_theta)
                        for _ in range(n))
            layer_idx += n
            if s == num_stages - 1:
                mods.append(LlamaHead(H, vocab_size))
            stages.append(_Stage(mods))
    model = StagedModel(stages)
    model.max_pos = max_pos
    return init_weights(model)
