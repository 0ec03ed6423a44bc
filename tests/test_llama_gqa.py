"""Grouped-query LLaMA attention: LlamaAttention with num_kv_heads against
an explicit fp64 composition on the CPU, the llama-tiny-gqa config, and the
packed RoPE + GQA flash attention Function against apply_rope +
flash_attention on the GPU."""

import pytest
import torch

from easyparallellibrary_amd.models import llama
from tests import kernel_refs as kr

F64 = torch.float64


def _rot(x, theta):
    """HF half-split rotation of [B, N, S, D] in x's dtype"""
    s, d = x.shape[-2], x.shape[-1]
    inv = theta ** (-torch.arange(d // 2, dtype=F64) / (d // 2))
    ang = torch.arange(s, dtype=F64)[:, None] * inv[None, :]
    c, sn = torch.cat([ang.cos()] * 2, -1), torch.cat([ang.sin()] * 2, -1)
    rot = torch.cat([-x[..., d // 2:], x[..., :d // 2]], -1)
    return x * c + rot * sn


def test_llama_attention_gqa_cpu_fp64():
    torch.manual_seed(0)
    hq, hkv, d, b, s = 2, 1, 64, 2, 9
    mod = llama.LlamaAttention(128, hq, num_kv_heads=hkv)
    assert mod.qkv.weight.shape == (256, 128)
    x = torch.randn(b, s, 128, requires_grad=True)
    dy = torch.randn(b, s, 128)
    mod(x).backward(dy)
    got = [mod(x).detach(), x.grad, mod.qkv.weight.grad, mod.proj.weight.grad]

    x64 = x.detach().to(F64).requires_grad_()
    wq = mod.qkv.weight.detach().to(F64).requires_grad_()
    wp = mod.proj.weight.detach().to(F64).requires_grad_()
    heads = (x64 @ wq.t()).view(b, s, hq + 2 * hkv, d).transpose(1, 2)
    q = _rot(heads[:, :hq], 10000.0)
    k = _rot(heads[:, hq:hq + hkv], 10000.0).repeat_interleave(hq // hkv, 1)
    v = heads[:, hq + hkv:].repeat_interleave(hq // hkv, 1)
    sc = (q @ k.transpose(-1, -2)) * d ** -0.5
    sc = sc.masked_fill(~torch.ones(s, s, dtype=torch.bool).tril(),
                        float("-inf"))
    y = (sc.softmax(-1) @ v).transpose(1, 2).reshape(b, s, hq * d) @ wp.t()
    y.backward(dy.to(F64))
    for g, w in zip(got, [y.detach(), x64.grad, wq.grad, wp.grad]):
        assert float((g.to(F64) - w).abs().max()) <= 1e-5 * float(
            w.abs().max())


def test_llama_tiny_gqa_config_and_mha_shape():
    model = llama.build_llama("llama-tiny-gqa", vocab_size=64)
    assert model.blocks[0].attn.qkv.weight.shape == (256, 128)
    ids = torch.randint(0, 64, (2, 10))
    model(ids).float().square().mean().backward()
    assert all(bool(torch.isfinite(p.grad).all())
               for p in model.parameters())
    assert llama.LlamaAttention(128, 2).qkv.weight.shape == (384, 128)
    assert llama.LLAMA_CONFIGS["llama3-8b"]["kv_heads"] == 8


@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv,d", [(4, 2, 64), (2, 1, 128)])
def test_rope_qkv_gqa_packed_gpu(hq, hkv, d):
    from easyparallellibrary_amd.ops.attention import flash_attention
    from easyparallellibrary_amd.ops.rope import (
        apply_rope, rope_qkv_flash_attention)
    b, s = 2, 200
    gen = torch.Generator().manual_seed(3)
    base = torch.randn(b, s, (hq + 2 * hkv) * d, generator=gen).bfloat16()
    dout = torch.randn(b, hq, s, d, generator=gen).bfloat16().cuda()

    xa = base.cuda().requires_grad_()
    parts = xa.view(b, s, hq + 2 * hkv, d).transpose(1, 2).split(
        [hq, hkv, hkv], dim=1)
    want = flash_attention(apply_rope(parts[0]), apply_rope(parts[1]),
                           parts[2], causal=True)
    want.backward(dout)

    xb = base.cuda().requires_grad_()
    flat = xb * 1          # a non-leaf, non-view buffer: the zero-copy form
    packed_bytes = flat.numel() * 2
    out_bytes, lse_bytes = b * hq * s * d * 2, b * hq * s * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = rope_qkv_flash_attention(flat, num_heads=hq, num_kv_heads=hkv)
    torch.cuda.synchronize()
    # in grad mode the Function holds out and lse (and the packed buffer
    # it was given); neither a kept nor a transient tensor of the packed
    # size fits under the limit
    slack = 16384
    assert out_bytes + lse_bytes + slack < packed_bytes
    assert torch.cuda.max_memory_allocated() - before <= \
        out_bytes + lse_bytes + slack
    got.backward(dout)

    # both sides round the same fp64 quantities: |got - want| <= the two
    # kernels' bounds added, taken on the rotated operands
    q, k, v = (t.detach().cpu().to(F64) for t in (
        apply_rope(parts[0]), apply_rope(parts[1]), parts[2]))
    ke, ve = (t.repeat_interleave(hq // hkv, 1) for t in (k, v))
    ref = kr.attn_ref(q, ke, ve, dout.cpu().to(F64), True, d ** -0.5)
    bound = kr.attn_bounds(ref, q, ke, ve, dout.cpu().to(F64), d ** -0.5)
    err = (got.detach().cpu().to(F64) - want.detach().cpu().to(F64)).abs()
    assert kr.attn_ratio(err, bound["out"]) <= 2 * kr.ATTN_FACTOR["out"]
    # input gradient, element-wise: dq | dk (summed over the group) | dv.
    # The rotation back mixes element i of a q / k head with element
    # i +- D/2 (|cos|, |sin| <= 1), so its bound is the sum of the two; v
    # is not rotated.  Each path may use ATTN_FACTOR x the bound, and each
    # rounds the stored gradient to bf16 once more after rotating it.
    def rot(e):
        return e + e.roll(d // 2, -1)
    gb = torch.cat([rot(bound["dq"]),
                    rot(bound["dk"].view(b, hkv, hq // hkv, s, d).sum(2)),
                    bound["dv"].view(b, hkv, hq // hkv, s, d).sum(2)], 1)

    def heads(t):
        return t.cpu().to(F64).view(b, s, hq + 2 * hkv, d).transpose(1, 2)
    gerr = (heads(xb.grad) - heads(xa.grad)).abs()
    lim = 2 * kr.ATTN_FACTOR["dq"] * gb + \
        2 * kr.U_BF16 * heads(xa.grad).abs()
    print("GQA-ROPE grad err / limit {:.3f}".format(
        kr.attn_ratio(gerr, lim)))
    assert bool((gerr <= lim).all()), kr.attn_ratio(gerr, lim)
    assert bool(torch.isfinite(xb.grad).all())
