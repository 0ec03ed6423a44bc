"""Right-padded batches from the Python ops up to BERT: seqlens_from_mask,
the torch fallback's semantics, the model plumbing (SelfAttention, Block,
BertCore, build_bert, synthetic_mlm_batch) on the CPU, and on the GPU that
the lengths reach the native kernels and that nothing at a valid position
depends on the padding."""

import pytest
import torch
import torch.nn.functional as F


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def test_seqlens_from_mask():
    from easyparallellibrary_amd.ops.attention import seqlens_from_mask
    mask = torch.tensor([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0],
                         [1, 0, 0, 0, 0]])
    for m in (mask, mask.bool(), mask.float()):
        lens = seqlens_from_mask(m)
        assert lens.dtype == torch.int32
        assert lens.tolist() == [3, 5, 0, 1]


def _slice_attention(q, k, v, causal, scale, lens):
    """every sample alone at its own length; zeros elsewhere"""
    out = torch.zeros_like(q)
    for b, n in enumerate(lens):
        if n:
            out[b, :, :n] = F.scaled_dot_product_attention(
                q[b:b + 1, :, :n], k[b:b + 1, :, :n], v[b:b + 1, :, :n],
                is_causal=causal, scale=scale)[0]
    return out


@pytest.mark.parametrize("causal", [False, True])
def test_fallback_semantics(causal):
    from easyparallellibrary_amd.ops.attention import flash_attention
    torch.manual_seed(0)
    b, h, s, d = 4, 2, 9, 16
    lens = [9, 4, 0, 1]
    seqlens = torch.tensor(lens, dtype=torch.int32)
    q, k, v = (torch.randn(b, h, s, d, dtype=torch.float64,
                           requires_grad=True) for _ in range(3))
    dout = torch.randn(b, h, s, d, dtype=torch.float64)
    out = flash_attention(q, k, v, causal=causal, seqlens=seqlens)
    gq, gk, gv = torch.autograd.grad(out, [q, k, v], dout)
    q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ref = _slice_attention(q2, k2, v2, causal, d ** -0.5, lens)
    rq, rk, rv = torch.autograd.grad(ref, [q2, k2, v2], dout)
    for got, want in ((out, ref), (gq, rq), (gk, rk), (gv, rv)):
        assert bool(torch.isfinite(got).all())
        assert torch.allclose(got, want, atol=1e-12, rtol=0)
    for i, n in enumerate(lens):
        for t in (out, gq, gk, gv):
            assert not bool(t[i, :, n:].any())
    # lengths past seq clamp; the padding's content reaches nothing
    over = flash_attention(q, k, v, causal=causal, seqlens=seqlens + 100)
    dense = flash_attention(q, k, v, causal=causal)
    assert torch.allclose(over, dense, atol=1e-12, rtol=0)
    q3 = q.detach().clone()
    k3, v3 = k.detach().clone(), v.detach().clone()
    for i, n in enumerate(lens):
        for t in (q3, k3, v3):
            t[i, :, n:] = float("nan")
    again = flash_attention(q3, k3, v3, causal=causal, seqlens=seqlens)
    assert torch.equal(again, out.detach())
    with pytest.raises(ValueError, match="int32"):
        flash_attention(q, k, v, seqlens=seqlens.long())
    with pytest.raises(ValueError, match="int32"):
        flash_attention(q, k, v, seqlens=seqlens[:2])


def test_build_bert_refuses_pad_id_with_stages():
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models import bert
    epl.init()
    with pytest.raises(ValueError, match="stage"):
        bert.build_bert("bert-tiny", vocab_size=64, max_pos=16,
                        num_stages=2, pad_token_id=0)
    model = bert.build_bert("bert-tiny", vocab_size=64, max_pos=16,
                            pad_token_id=0)
    assert model.pad_token_id == 0
    assert bert.build_bert("bert-tiny", vocab_size=64,
                           max_pos=16).pad_token_id is None


def test_synthetic_mlm_batch_defaults_and_lengths():
    from easyparallellibrary_amd.models.bert import synthetic_mlm_batch
    # what the function produced before it knew lengths
    g = torch.Generator(device="cpu")
    g.manual_seed(11)
    ids = torch.randint(0, 1000, (4, 32), generator=g)
    targets = ids.clone()
    mask = torch.rand(4, 32, generator=g) < 0.15
    targets[~mask] = -100
    ids[mask] = 103
    got_ids, got_tgt = synthetic_mlm_batch(4, 32, 1000, seed=11)
    assert torch.equal(got_ids, ids) and torch.equal(got_tgt, targets)
    lens = [32, 7, 0, 19]
    pid, ptgt = synthetic_mlm_batch(4, 32, 1000, seed=11, lengths=lens,
                                    pad_token_id=5)
    for b, n in enumerate(lens):
        assert torch.equal(pid[b, :n], ids[b, :n])
        assert torch.equal(ptgt[b, :n], targets[b, :n])
        assert bool((pid[b, n:] == 5).all())
        assert bool((ptgt[b, n:] == -100).all())


def _padded_ids(lens, seq, vocab, pad, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(pad + 1, vocab, (len(lens), seq), generator=g)
    for b, n in enumerate(lens):
        ids[b, n:] = pad
    return ids


def test_bert_padded_batch_equals_samples_alone():
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models import bert
    epl.init()
    torch.manual_seed(3)
    seq, vocab, lens = 16, 64, [16, 9, 1, 12]
    model = bert.build_bert("bert-tiny", vocab_size=vocab, max_pos=seq,
                            pad_token_id=0).float().eval()
    ids = _padded_ids(lens, seq, vocab, 0, seed=5)
    with torch.no_grad():
        logits = model(ids)
        explicit = model(ids, seqlens=torch.tensor(lens, dtype=torch.int32))
        assert torch.equal(logits, explicit)
        for b, n in enumerate(lens):
            alone = model(ids[b:b + 1, :n])
            assert torch.allclose(logits[b, :n], alone[0], atol=1e-5,
                                  rtol=0), (b, n)
        # without the lengths the padding does leak into the valid rows
        model.pad_token_id = None
        assert not torch.allclose(model(ids)[1, :9], logits[1, :9],
                                  atol=1e-5, rtol=0)


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
def _attention_module(hidden=128, heads=2):
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models.transformer import SelfAttention
    epl.init()
    torch.manual_seed(21)
    return SelfAttention(hidden, heads).to("cuda", torch.bfloat16).train()


@pytest.mark.gpu
def test_selfattention_lengths_stay_native():
    """the lengths arrive at _C.attn_fwd / _C.attn_bwd: no SDPA fallback,
    no dense mask"""
    import easyparallellibrary_amd.ops.attention as A
    m = _attention_module()
    x = torch.randn(3, 200, 128, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    seqlens = torch.tensor([200, 77, 0], dtype=torch.int32, device="cuda")
    real = A.native_ext()
    seen = {}

    class Spy:
        def __getattr__(self, name):
            return getattr(real, name)

        def attn_fwd(self, *args, **kwargs):
            seen["fwd"] = args[-1] if len(args) == 12 \
                else kwargs.get("seqlens")
            return real.attn_fwd(*args, **kwargs)

        def attn_bwd(self, *args, **kwargs):
            seen["bwd"] = args[-1] if len(args) == 17 \
                else kwargs.get("seqlens")
            return real.attn_bwd(*args, **kwargs)

    orig_ext, orig_sdpa = A.native_ext, F.scaled_dot_product_attention

    def no_sdpa(*args, **kwargs):
        raise AssertionError("padded batch left the native kernels")

    A.native_ext = lambda: Spy()
    F.scaled_dot_product_attention = no_sdpa
    try:
        y = m(x, seqlens=seqlens)
        y.float().sum().backward()
    finally:
        A.native_ext = orig_ext
        F.scaled_dot_product_attention = orig_sdpa
    for key in ("fwd", "bwd"):
        got = seen.get(key)
        assert got is not None, (key, seen)
        assert got.dtype == torch.int32
        assert got.data_ptr() == seqlens.data_ptr(), key
    assert bool(torch.isfinite(y.float()).all())
    assert bool(torch.isfinite(x.grad.float()).all())


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True])
def test_selfattention_against_masked_fp32(causal):
    """the attention inside SelfAttention, from the bf16 qkv it was given:
    output within 3e-2 and qkv gradient within 6e-2 of the fp32 masked
    reference; padded rows exactly zero"""
    m = _attention_module()
    m.causal = causal
    b, s, nh, d = 3, 200, 2, 64
    lens = [200, 77, 0]
    seqlens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    x = torch.randn(b, s, 128, device="cuda", dtype=torch.bfloat16)
    store = {}

    def keep_qkv(mod, inp, out):
        out.retain_grad()
        store["qkv"] = out

    def keep_o(mod, inp):
        inp[0].retain_grad()
        store["o"] = inp[0]

    h1 = m.qkv.register_forward_hook(keep_qkv)
    h2 = m.proj.register_forward_pre_hook(keep_o)
    try:
        y = m(x, seqlens=seqlens)
    finally:
        h1.remove()
        h2.remove()
    g = torch.Generator(device="cuda").manual_seed(4)
    y.backward(torch.randn(y.shape, device="cuda", generator=g).to(y.dtype))
    torch.cuda.synchronize()
    qkv, o = store["qkv"], store["o"]

    ref_in = qkv.detach().float().requires_grad_(True)
    r = ref_in.reshape(b, s, 3, nh, d)
    qf, kf, vf = (r[:, :, i].transpose(1, 2) for i in range(3))
    pos = torch.arange(s, device="cuda")
    keys = pos[None, :] < seqlens.clamp(min=1)[:, None]
    allowed = keys[:, None, None, :]
    if causal:
        allowed = allowed & (pos[None, :] <= pos[:, None])
    sc = (qf @ kf.transpose(-1, -2)) * d ** -0.5
    p = sc.masked_fill(~allowed, float("-inf")).softmax(-1)
    rows = (pos[None, :] < seqlens[:, None])[:, None, :, None]
    ref = torch.where(rows, p @ vf, torch.zeros(()).to(vf))
    ref = ref.transpose(1, 2).reshape(b, s, nh * d)
    ref.backward(o.grad.float())
    torch.cuda.synchronize()
    assert torch.allclose(o.float(), ref, atol=3e-2, rtol=0), (
        (o.float() - ref).abs().max())
    assert torch.allclose(qkv.grad.float(), ref_in.grad, atol=6e-2, rtol=0), (
        (qkv.grad.float() - ref_in.grad).abs().max())
    for i, n in enumerate(lens):
        assert not bool(o[i, n:].any())
        assert not bool(qkv.grad[i, n:].any())


def _tiny_bert(pad_token_id=None):
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models import bert
    epl.init()
    torch.manual_seed(9)
    return bert.build_bert("bert-tiny", vocab_size=512, max_pos=200,
                           pad_token_id=pad_token_id)


@pytest.mark.gpu
def test_bert_ignores_ids_at_padded_positions():
    from easyparallellibrary_amd.ops.distributed_losses import (
        ParallelCrossEntropy)
    seq, vocab, lens = 200, 512, [200, 130, 64, 1]
    model = _tiny_bert().to("cuda", torch.bfloat16).train()
    loss_fn = ParallelCrossEntropy()
    seqlens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    g = torch.Generator().manual_seed(1)
    targets = torch.randint(0, vocab, (len(lens), seq), generator=g)
    rows = torch.arange(seq)[None, :] < torch.tensor(lens)[:, None]
    targets[~rows] = -100
    targets = targets.cuda()
    runs = []
    base = _padded_ids(lens, seq, vocab, 0, seed=5)
    for seed in (5, 6):
        # the two runs differ in the ids at the padded positions only
        filler = torch.randint(0, vocab, base.shape,
                               generator=torch.Generator().manual_seed(seed))
        ids = torch.where(rows, base, filler).cuda()
        model.zero_grad(set_to_none=True)
        logits = model(ids, seqlens=seqlens)
        loss = loss_fn(logits, targets)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((ids.cpu(), logits.detach()[rows.cuda()].clone(),
                     loss.detach().clone(),
                     {n: p.grad.clone() for n, p in model.named_parameters()}))
    (ids_a, la, loss_a, ga), (ids_b, lb, loss_b, gb) = runs
    assert torch.equal(ids_a[rows], ids_b[rows])
    assert not torch.equal(ids_a[~rows], ids_b[~rows])
    assert torch.equal(la, lb)
    assert torch.equal(loss_a, loss_b) and bool(torch.isfinite(loss_a))
    tables = ("embeddings.tok.weight", "embeddings.pos.weight")
    assert set(tables) <= set(ga)
    for name in ga:
        assert bool(torch.isfinite(ga[name].float()).all()), name
        if name not in tables:   # their backward adds with atomics
            assert torch.equal(ga[name], gb[name]), name


@pytest.mark.gpu
def test_engine_step_on_padded_batch():
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models import bert
    from easyparallellibrary_amd.ops.distributed_losses import (
        ParallelCrossEntropy)
    model = _tiny_bert(pad_token_id=0)
    loss_fn = ParallelCrossEntropy()
    engine = epl.Engine(model, loss_fn=lambda o, t: loss_fn(o, t),
                        optimizer="adamw", lr=1e-4, dtype=torch.bfloat16)
    lens = [200, 130, 0, 1]
    ids, tgt = bert.synthetic_mlm_batch(4, 200, 512, device=engine.device,
                                        seed=7, mask_frac=0.5, lengths=lens,
                                        pad_token_id=0)
    # a valid position never holds the pad id (lengths come from the ids)
    rows = (torch.arange(200)[None, :] < torch.tensor(lens)[:, None]).to(
        ids.device)
    ids = torch.where(rows & (ids == 0), torch.ones_like(ids), ids)
    assert (ids != 0).sum(1).tolist() == lens
    loss = engine.train_step(ids, tgt)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)), loss
    assert engine.flat_groups
    for fg in engine.flat_groups:
        assert not bool(torch.isnan(fg.grad_arena.float()).any())
