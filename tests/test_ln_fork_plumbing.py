"""The forked LayerNorm output (FusedLayerNorm.forward_pair) through the
post-LN models: a LayerNorm output with two consumers travels as two
tensors on one storage, so the LN backward receives both gradients and
adds them itself instead of autograd's add kernel.

* CPU, fp32: a 2-block post-LN BertCore (hidden 64) with the fork on and
  off gives torch.equal loss and parameter gradients (the fallback adds
  the two gradients in the compute dtype, which is what autograd did).
* GPU, bf16: the same model with the fork on and off, each against an fp64
  run on the CPU; per parameter, the max-abs error with the fork is at
  most 1.25 x the error without it plus one bf16 ulp of the gradient's max
  magnitude (the rule of test_attention_bwd_tiles_gpu.py: the kernel adds
  in fp32 where autograd rounded the sum to bf16, a rounding moved, while
  a lost or doubled gradient is an O(1) error).
* Where the pair cannot travel the model still trains: a block behind the
  checkpoint wrapper, a replaced block, a 2-stage build_bert; and the
  pre-LN block refuses the pair.
* The second copy alone, or neither, used: backward copes with None.
"""

import math

import pytest
import torch

from easyparallellibrary_amd.models import bert
from easyparallellibrary_amd.models.transformer import Block
from easyparallellibrary_amd.ops import layer_norm as ln_mod
from easyparallellibrary_amd.ops.distributed_losses import (
    ParallelCrossEntropy)

CFG = dict(layers=2, hidden=64, heads=2, ffn=128)
VOCAB, SEQ, BATCH = 128, 16, 3


@pytest.fixture
def fork_switch():
    saved = ln_mod._LN_BWD_FORK

    def set_fork(on):
        ln_mod._LN_BWD_FORK = on

    yield set_fork
    ln_mod._LN_BWD_FORK = saved


def make_model(seed=0, **kw):
    torch.manual_seed(seed)
    model = bert.build_bert(CFG, vocab_size=VOCAB, max_pos=SEQ, **kw)
    # biases and LN parameters off their init, so every gradient matters
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    return model


def loss_and_grads(model, device="cpu"):
    ids, tgt = bert.synthetic_mlm_batch(BATCH, SEQ, VOCAB, device=device,
                                        seed=1)
    model.zero_grad(set_to_none=True)
    loss = ParallelCrossEntropy()(model(ids), tgt)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    assert all(torch.isfinite(g).all() for g in grads.values())
    return loss.detach(), grads


def test_fork_on_off_equal_cpu_fp32(fork_switch):
    model = make_model()
    fork_switch(True)
    loss1, g1 = loss_and_grads(model)
    fork_switch(False)
    loss0, g0 = loss_and_grads(model)
    assert torch.equal(loss1, loss0)
    assert g1.keys() == g0.keys() and len(g1) > 20
    for name in g1:
        assert torch.equal(g1[name], g0[name]), name


def test_forward_pair_shares_storage_and_counts(fork_switch):
    lnm = ln_mod.FusedLayerNorm(64)
    x = torch.randn(5, 64, requires_grad=True)
    fork_switch(True)
    a, b = lnm.forward_pair(x)
    assert a is not b and a.data_ptr() == b.data_ptr()
    assert torch.equal(a, b)
    # either copy alone, both, or none used
    want = torch.autograd.grad(lnm(x).sum() * 2, x)[0]
    got = torch.autograd.grad(a.sum() + b.sum(), x)[0]
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)
    a, b = lnm.forward_pair(x)
    only_b = torch.autograd.grad(b.sum(), x)[0]
    assert torch.allclose(only_b * 2, want, rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        a, b = lnm.forward_pair(x)
        assert a is b
    fork_switch(False)
    a, b = lnm.forward_pair(x)
    assert a is b


def test_kill_switch_env_read_once():
    """EPL_LN_BWD_FORK=0 in a fresh process turns the fork off"""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from easyparallellibrary_amd.ops import layer_norm as m; "
            "print(int(m._LN_BWD_FORK))")
    for value, want in (("0", "0"), ("1", "1"), (None, "1")):
        env = dict(os.environ)
        env.pop("EPL_LN_BWD_FORK", None)
        if value is not None:
            env["EPL_LN_BWD_FORK"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=repo, env=env,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip().splitlines()[-1] == want


class _Replaced(torch.nn.Module):
    """a block the model does not know: takes and returns one tensor"""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x)


@pytest.mark.parametrize("where", [0, 1])
@pytest.mark.parametrize("kind", ["checkpoint", "replaced"])
def test_fallback_blocks_match_plain_model(fork_switch, kind, where):
    """a wrapped or replaced block computes what the plain model computes
    (fp32 on the CPU: equal up to the order of one gradient add)"""
    from easyparallellibrary_amd.runtime.gc import CheckpointWrapper
    fork_switch(True)
    plain = make_model()
    loss_p, g_p = loss_and_grads(plain)
    model = make_model()
    wrap = CheckpointWrapper if kind == "checkpoint" else _Replaced
    model.blocks[where] = wrap(model.blocks[where])
    model.train()
    loss_w, g_w = loss_and_grads(model)
    assert torch.equal(loss_w, loss_p)
    for name, g in g_p.items():
        wname = name.replace("blocks.%d." % where,
                             "blocks.%d.inner." % where)
        assert torch.allclose(g_w[wname], g, rtol=1e-5, atol=1e-7), name


def test_two_stage_bert_trains(fork_switch):
    fork_switch(True)
    model = make_model(num_stages=2)
    loss, grads = loss_and_grads(model)
    assert math.isfinite(float(loss)) and len(grads) > 20
    assert all(float(g.abs().max()) > 0 for n, g in grads.items()
               if "tok" not in n and "pos" not in n)


def test_pre_ln_block_refuses_the_pair():
    blk = Block(64, 2, 128, pre_ln=True)
    x = torch.randn(2, 4, 64)
    assert blk(x).shape == x.shape
    with pytest.raises(ValueError):
        blk(x, pair_out=True)
    with pytest.raises(ValueError):
        blk(x, x_res=x.clone())


def bf16_ulp(x):
    """spacing of bf16 (8 significand bits) at magnitude x"""
    return 2.0 ** (math.floor(math.log2(x)) - 7) if x > 0 else 0.0


@pytest.mark.gpu
def test_fork_on_off_bf16_gpu_against_fp64(fork_switch):
    ref_model = make_model().double()
    fork_switch(False)
    _, g_ref = loss_and_grads(ref_model)
    dev_model = make_model().to("cuda:0").to(torch.bfloat16)
    errs = {}
    for on in (False, True):
        fork_switch(on)
        loss, grads = loss_and_grads(dev_model, device="cuda:0")
        assert math.isfinite(float(loss))
        errs[on] = {n: float((g.cpu().double() - g_ref[n]).abs().max())
                    for n, g in grads.items()}
    bad = []
    for name, ref in g_ref.items():
        refmax = float(ref.abs().max())
        bound = 1.25 * errs[False][name] + bf16_ulp(refmax)
        print("FORK-ERR %-40s new %.3e old %.3e bound %.3e max|ref| %.3e"
              % (name, errs[True][name], errs[False][name], bound, refmax))
        if not errs[True][name] <= bound:
            bad.append((name, errs[True][name], bound))
    assert not bad, bad[:8]
