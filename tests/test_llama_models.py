"""The LLaMA model family (models/llama.py) and its ops.

CPU: fp32 llama-tiny against an independent plain-torch LLaMA written here
(weights copied), apply_rope's gradient, gradient checkpointing, PP2 1F1B
over gloo against the serial run, and the fp32 RoPE tables surviving a bf16
Engine.  GPU (marked): the block really runs the native kernels, the native
bf16 path is no further from an fp32 run than twice the torch bf16 path,
Engine steps train, and the hipGraph-captured step equals the eager one.
"""

import copy
import math

import pytest
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from tests.utils import run_multiprocess

VOCAB = 512
TINY = dict(layers=2, hidden=128, heads=2, ffn=352)


def _lm_loss(out, tgt):
    return F.cross_entropy(out.reshape(-1, out.shape[-1]).float(),
                           tgt.reshape(-1))


def _build_tiny(num_stages=1, seed=5):
    from easyparallellibrary_amd.models import llama
    torch.manual_seed(seed)
    return llama.build_llama(TINY, vocab_size=VOCAB, max_pos=64,
                             num_stages=num_stages)


# ---- an independent LLaMA in plain torch ----------------------------------
def _plain_rms(x, w, eps=1e-5):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def _plain_rope(x, theta=10000.0):
    """x: [B, H, S, D]; HF rotate_half with tables made here"""
    seq, d = x.shape[-2], x.shape[-1]
    inv = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.float64) / d))
    ang = torch.outer(torch.arange(seq, dtype=torch.float64), inv)
    emb = torch.cat([ang, ang], dim=-1)
    cos, sin = emb.cos().to(x.dtype), emb.sin().to(x.dtype)
    x1, x2 = x[..., :d // 2], x[..., d // 2:]
    return x * cos + torch.cat([-x2, x1], dim=-1) * sin


def _plain_llama(p, ids, layers, heads):
    x = p["embeddings.tok.weight"][ids]
    b, s, h = x.shape
    d = h // heads
    causal = torch.tril(torch.ones(s, s, dtype=torch.bool))
    for i in range(layers):
        pre = "blocks.%d." % i
        y = _plain_rms(x, p[pre + "rms1.weight"])
        qkv = (y @ p[pre + "attn.qkv.weight"].t()).reshape(b, s, 3, heads, d)
        q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))
        q, k = _plain_rope(q), _plain_rope(k)
        sc = (q @ k.transpose(-1, -2)) / math.sqrt(d)
        sc = sc.masked_fill(~causal, float("-inf"))
        o = (torch.softmax(sc, dim=-1) @ v).transpose(1, 2).reshape(b, s, h)
        x = x + o @ p[pre + "attn.proj.weight"].t()
        y = _plain_rms(x, p[pre + "rms2.weight"])
        gu = y @ p[pre + "fc12.weight"].t()
        f = gu.shape[-1] // 2
        x = x + (F.silu(gu[..., :f]) * gu[..., f:]) @ p[pre + "fc2.weight"].t()
    return _plain_rms(x, p["head.norm.weight"]) @ p["head.proj.weight"].t()


def _batch(b=2, s=24, seed=3):
    from easyparallellibrary_amd.models.llama import synthetic_lm_batch
    return synthetic_lm_batch(b, s, VOCAB, seed=seed)


def test_llama_tiny_fp32_equals_plain_torch():
    model = _build_tiny()
    # weights off their init so that every norm weight matters
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if name.endswith("rms1.weight") or name.endswith("rms2.weight") \
                    or name.endswith("norm.weight"):
                prm.add_(0.1 * torch.randn(prm.shape, generator=gen))
    ids, tgt = _batch()
    params = {n: p.detach().clone().requires_grad_()
              for n, p in model.named_parameters()}
    assert set(params) == {
        "embeddings.tok.weight", "head.norm.weight", "head.proj.weight"} | {
        "blocks.%d.%s.weight" % (i, m) for i in range(2) for m in (
            "rms1", "attn.qkv", "attn.proj", "rms2", "fc12", "fc2")}
    logits = model(ids)
    _lm_loss(logits, tgt).backward()
    want = _plain_llama(params, ids, TINY["layers"], TINY["heads"])
    _lm_loss(want, tgt).backward()
    assert float((logits - want).detach().abs().max()) <= 1e-5
    for name, prm in model.named_parameters():
        g, w = prm.grad, params[name].grad
        assert float((g - w).abs().max()) <= 1e-5 * max(
            1.0, float(w.abs().max())), name


def test_apply_rope_gradient_is_autograd_of_the_composition():
    from easyparallellibrary_amd.ops.rope import apply_rope
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 17, 64, generator=gen, dtype=torch.float64)
    g = torch.randn(2, 3, 17, 64, generator=gen, dtype=torch.float64)
    a = x.clone().requires_grad_()
    b = x.clone().requires_grad_()
    ya = apply_rope(a)
    yb = _plain_rope(b)
    # the op reads fp32 tables, the composition here fp64 ones
    assert float((ya - yb).abs().max()) <= 2.0 ** -22 * float(x.abs().max())
    ya.backward(g)
    yb.backward(g)
    assert float((a.grad - b.grad).abs().max()) <= 2.0 ** -22 * float(
        g.abs().max())
    # a later window of positions is the rotation of a longer sequence
    long = apply_rope(torch.cat([torch.zeros(2, 3, 5, 64, dtype=x.dtype), x],
                                dim=2))
    assert torch.equal(apply_rope(x, pos0=5), long[:, :, 5:])


def _block_grads(block, x, mode):
    block.zero_grad(set_to_none=True)
    xin = x.clone().requires_grad_()
    if mode is None:
        y = block(xin)
    else:
        y = checkpoint(block, xin, use_reentrant=mode)
    y.float().square().sum().backward()
    return [xin.grad] + [p.grad for p in block.parameters()]


def _check_checkpoint_bitwise(block, x):
    plain = _block_grads(block, x, None)
    for mode in (True, False):
        again = _block_grads(block, x, mode)
        for a, b in zip(plain, again):
            assert a is not None and torch.equal(a, b), mode


def test_checkpoint_leaves_gradients_bitwise_unchanged_cpu():
    from easyparallellibrary_amd.models.llama import LlamaBlock
    torch.manual_seed(1)
    block = LlamaBlock(128, 2, 352)
    _check_checkpoint_bitwise(block, torch.randn(2, 16, 128))


def _llama_worker(rank, world, stages):
    import easyparallellibrary_amd as epl
    epl.init(epl.Config({"pipeline.num_micro_batch": 4}))
    model = _build_tiny(num_stages=stages)
    engine = epl.Engine(model, loss_fn=_lm_loss, optimizer="adamw", lr=1e-2)
    ids, tgt = _batch(b=8, s=16)
    out = []
    for _ in range(3):
        loss = engine.train_step(ids, tgt)
        out.append(None if loss is None else float(loss))
    return out


def test_llama_pp2_1f1b_matches_serial():
    serial = run_multiprocess(_llama_worker, world=1, args=(1,))[0]
    pp = run_multiprocess(_llama_worker, world=2, args=(2,))
    assert pp[0][0] is None            # the loss lives on the last stage
    assert all(abs(a - b) < 1e-5 for a, b in zip(serial, pp[1])), (
        serial, pp[1])
    assert serial[-1] < serial[0]


def test_rope_tables_stay_fp32_under_a_bf16_engine():
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.ops import rope
    epl.init()
    model = _build_tiny()
    engine = epl.Engine(model, loss_fn=_lm_loss, optimizer="adamw", lr=1e-3,
                        dtype=torch.bfloat16)
    ids, _ = _batch()
    out = engine.eval_step(ids.to(engine.device))
    assert out.dtype == torch.bfloat16
    # nothing of the tables is a module buffer that .to(dtype) could round
    assert list(model.buffers()) == []
    hits = [v for k, v in rope._TABLES.items() if k[1] == 64]
    assert hits
    for cos, sin in hits:
        assert cos.dtype == torch.float32 and sin.dtype == torch.float32
    cos, _ = rope.rope_tables(engine.device, 64)
    # an angle bf16 cannot hold: position 1000 of the slowest pair
    assert float(cos[1000, -1]) != float(cos[1000, -1].bfloat16())


def test_llama_configs():
    from easyparallellibrary_amd.models.llama import LLAMA_CONFIGS
    assert LLAMA_CONFIGS["llama-tiny"] == TINY
    assert LLAMA_CONFIGS["llama-1b"] == dict(layers=16, hidden=2048, heads=16,
                                             ffn=5632)
    assert LLAMA_CONFIGS["llama-7b"] == dict(layers=32, hidden=4096, heads=32,
                                             ffn=11008)
    for cfg in LLAMA_CONFIGS.values():
        assert cfg["hidden"] // cfg["heads"] in (64, 128)
        assert cfg["ffn"] % 8 == 0 and cfg["hidden"] <= 8192


def test_llama_example_tiny_cpu():
    """examples/train_llama_dp.py runs end-to-end in tiny mode on CPU"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(
        [sys.executable, os.path.join(root, "examples", "train_llama_dp.py")],
        env=dict(os.environ, EPL_EXAMPLE_TINY="1"), capture_output=True,
        text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "step 9" in r.stdout, r.stdout[-500:]


# ---- GPU ------------------------------------------------------------------
@pytest.mark.gpu
def test_llama_block_runs_the_native_kernels(monkeypatch):
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd import _C
    from easyparallellibrary_amd.models.llama import LlamaBlock
    from easyparallellibrary_amd.ops import rope, swiglu
    epl.init()
    calls = {}
    for name in ("rms_norm_fwd", "rms_norm_bwd", "rope_", "attn_fwd",
                 "attn_bwd", "swiglu_fwd", "swiglu_bwd"):
        def counted(*a, _fn=getattr(_C, name), _name=name, **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **kw)
        monkeypatch.setattr(_C, name, counted)

    def refuse(*a, **kw):
        raise AssertionError("torch fallback on the native path")

    monkeypatch.setattr(rope, "_rope_torch", refuse)
    monkeypatch.setattr(swiglu.F, "silu", refuse)
    monkeypatch.setattr(F, "scaled_dot_product_attention", refuse)
    torch.manual_seed(0)
    block = LlamaBlock(128, 2, 352).to("cuda", torch.bfloat16)
    x = torch.randn(2, 64, 128, device="cuda",
                    dtype=torch.bfloat16).requires_grad_()
    y = block(x)
    y.float().square().sum().backward()
    torch.cuda.synchronize()
    assert calls == dict(rms_norm_fwd=2, rms_norm_bwd=2, rope_=2, attn_fwd=1,
                         attn_bwd=1, swiglu_fwd=1, swiglu_bwd=1), calls
    assert bool(torch.isfinite(y.float()).all())
    assert bool(torch.isfinite(x.grad.float()).all())
    for p in block.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all())


@pytest.mark.gpu
def test_checkpoint_leaves_gradients_bitwise_unchanged_gpu():
    """the in-place RoPE + attention Function under both checkpoint forms"""
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models.llama import LlamaBlock
    epl.init()
    torch.manual_seed(1)
    block = LlamaBlock(128, 2, 352).to("cuda", torch.bfloat16)
    x = torch.randn(2, 64, 128, device="cuda", dtype=torch.bfloat16)
    _check_checkpoint_bitwise(block, x)


def _logits_and_grads(model, ids, tgt):
    model.zero_grad(set_to_none=True)
    logits = model(ids)
    _lm_loss(logits, tgt).backward()
    torch.cuda.synchronize()
    return (logits.detach().float(),
            {n: p.grad.detach().float() for n, p in model.named_parameters()})


@pytest.mark.gpu
def test_llama_native_bf16_no_further_from_fp32_than_twice_torch_bf16():
    """e_native = |native bf16 - fp32|, e_torch = |torch-path bf16 - fp32|
    in max-norm, for the logits and every parameter gradient: both bf16
    paths round, in different places, and the torch path more often, so
    e_native <= 2 e_torch allows for placement only.  No fixed tolerance."""
    import easyparallellibrary_amd as epl
    epl.init()
    ref_model = _build_tiny().cuda()
    ids, tgt = (t.cuda() for t in _batch(b=4, s=64))
    want_logits, want = _logits_and_grads(ref_model, ids, tgt)
    low = copy.deepcopy(ref_model).to(torch.bfloat16)
    nat_logits, nat = _logits_and_grads(low, ids, tgt)
    epl.init(epl.Config({"kernel.fused": False}))
    tor_logits, tor = _logits_and_grads(low, ids, tgt)
    bad = []
    pairs = [("logits", nat_logits, tor_logits, want_logits)] + [
        (n, nat[n], tor[n], want[n]) for n in want]
    for name, a, b, w in pairs:
        e_nat = float((a - w).abs().max())
        e_tor = float((b - w).abs().max())
        print("LLAMA-ERR %-28s native %.3e torch %.3e ratio %.2f" % (
            name, e_nat, e_tor, e_nat / e_tor if e_tor else float("inf")))
        if not e_nat <= 2 * e_tor:
            bad.append((name, e_nat, e_tor))
    assert not bad, bad


def _train(graphed, steps=8):
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.ops.distributed_losses import (
        ParallelCrossEntropy)
    epl.init(epl.Config({"kernel.hip_graph": graphed}))
    model = _build_tiny()
    engine = epl.Engine(model, loss_fn=ParallelCrossEntropy(),
                        optimizer="adamw", lr=1e-3, dtype=torch.bfloat16)
    ids, tgt = (t.to(engine.device) for t in _batch(b=4, s=64, seed=11))
    losses = [float(engine.train_step(ids, tgt)) for _ in range(steps)]
    torch.cuda.synchronize()
    return engine, losses


@pytest.mark.gpu
def test_llama_tiny_engine_steps_train():
    _, losses = _train(False, steps=2)
    assert all(math.isfinite(v) for v in losses)
    assert losses[1] < losses[0], losses


@pytest.mark.gpu
def test_llama_hipgraph_step_matches_eager():
    from easyparallellibrary_amd.runtime.hipgraph import HipGraphStep
    engine_g, losses_g = _train(True)
    assert isinstance(engine_g._hipgraph, HipGraphStep)
    assert engine_g._hipgraph.graph is not None
    engine_e, losses_e = _train(False)
    assert engine_e._hipgraph is False
    for lg, le in zip(losses_g, losses_e):
        assert abs(lg - le) <= 0.05 * abs(le) + 1e-2, (losses_g, losses_e)
    assert losses_g[-1] < losses_g[0]
