"""Load-balance and z losses of ExpertParallelMLP on the CPU: the gradients
the layer injects equal autograd of the explicitly written total loss,
defaults are bit-identical to the layer without the arguments, gradient
checkpointing and a pipeline stage boundary change nothing, and a short
training run shows the balance loss doing its job."""

import torch
import torch.nn as nn
import torch.utils.checkpoint

from easyparallellibrary_amd.ops import moe
from easyparallellibrary_amd.ops.moe import ExpertParallelMLP
from tests.utils import run_multiprocess

HIDDEN, FFN, EXPERTS, TOKENS = 16, 32, 4, 24
C_BAL, C_Z = 0.1, 0.01


def _layer(seed=3, **kw):
    torch.manual_seed(seed)
    return ExpertParallelMLP(HIDDEN, FFN, EXPERTS, top_k=2, **kw)


def _inputs(seed=4):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(TOKENS, HIDDEN, generator=gen)
    tgt = torch.randn(TOKENS, HIDDEN, generator=gen)
    return x, tgt


def _explicit_aux(layer, x):
    """L_bal and L_z of the module docstring, in plain torch"""
    z = layer.gate(x).float()
    n, e = z.shape
    p = z.softmax(dim=-1)
    topi = z.topk(layer.top_k, dim=-1).indices
    f = torch.bincount(topi.reshape(-1), minlength=e).float() / (
        n * layer.top_k)
    l_bal = e * (f * p.mean(dim=0)).sum()
    l_z = (torch.logsumexp(z, dim=-1) ** 2).mean()
    return l_bal, l_z


def _grads(layer):
    return {n: p.grad.clone() for n, p in layer.named_parameters()}


def _check_against_explicit(scale):
    x, tgt = _inputs()
    layer = _layer(aux_loss_coef=C_BAL, z_loss_coef=C_Z)
    plain = _layer()
    plain.load_state_dict(layer.state_dict())
    moe.set_aux_loss_scale(scale)
    try:
        out = layer(x)
        ((out * tgt).sum() * scale).backward()
    finally:
        moe.set_aux_loss_scale(1.0)
    out_p = plain(x)
    l_bal, l_z = _explicit_aux(plain, x)
    (((out_p * tgt).sum() + C_BAL * l_bal + C_Z * l_z) * scale).backward()
    assert torch.allclose(out, out_p, rtol=1e-5, atol=1e-8)
    assert torch.allclose(layer.last_balance_loss, l_bal.detach(),
                          rtol=1e-5)
    assert torch.allclose(layer.last_z_loss, l_z.detach(), rtol=1e-5)
    assert int(layer.last_expert_counts.sum()) == TOKENS * 2
    got, want = _grads(layer), _grads(plain)
    # the aux part of the gate gradient is there at all
    noaux = _layer()
    noaux.load_state_dict(layer.state_dict())
    ((noaux(x) * tgt).sum() * scale).backward()
    assert not torch.allclose(got["gate.weight"],
                              noaux.gate.weight.grad, rtol=1e-3, atol=0)
    for name in want:
        assert torch.allclose(got[name], want[name], rtol=1e-4,
                              atol=1e-6 * scale), (
            name, (got[name] - want[name]).abs().max())


def test_gradients_equal_explicit_total_loss():
    _check_against_explicit(1.0)


def test_gradients_with_loss_scale():
    _check_against_explicit(128.0)


def test_defaults_are_bit_identical():
    x, tgt = _inputs()
    a = ExpertParallelMLP
    torch.manual_seed(3)
    base = a(HIDDEN, FFN, EXPERTS, top_k=2)
    zero = _layer(aux_loss_coef=0.0, z_loss_coef=0.0, fused_router=None)
    outs = []
    for layer in (base, zero):
        out = layer(x)
        (out * tgt).sum().backward()
        outs.append(out)
        assert layer.last_balance_loss is None
    assert torch.equal(outs[0], outs[1])
    for (n, p), (_, q) in zip(base.named_parameters(),
                              zero.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    assert moe.moe_aux_losses(base) == dict(balance_loss=None, z_loss=None)


def test_aux_losses_helper_sums_layers():
    x, _ = _inputs()
    model = nn.Sequential(_layer(aux_loss_coef=C_BAL, z_loss_coef=C_Z),
                          _layer(seed=5, aux_loss_coef=C_BAL))
    model(x)
    got = moe.moe_aux_losses(model)
    assert torch.equal(got["balance_loss"], model[0].last_balance_loss +
                       model[1].last_balance_loss)
    assert torch.equal(got["z_loss"],
                       model[0].last_z_loss + model[1].last_z_loss)
    assert not got["balance_loss"].requires_grad


def test_checkpointing_leaves_gradients_unchanged():
    x, tgt = _inputs()
    want = None
    for mode in (None, False, True):
        layer = _layer(aux_loss_coef=C_BAL, z_loss_coef=C_Z)
        xx = x.clone().requires_grad_(True)
        if mode is None:
            out = layer(xx)
        else:
            out = torch.utils.checkpoint.checkpoint(layer, xx,
                                                    use_reentrant=mode)
        (out * tgt).sum().backward()
        got = _grads(layer)
        got["x"] = xx.grad.clone()
        if want is None:
            want = got
        for name in want:
            assert torch.equal(got[name], want[name]), (mode, name)


# ---- pipeline: the MoE layer on stage 0 -------------------------------------
PP_KW = dict(layers=2, hidden=32, heads=4, ffn=64, num_experts=4,
             vocab_size=128, max_pos=32, aux_loss_coef=C_BAL,
             z_loss_coef=C_Z)
PP_MICRO = 2


def _pp_data():
    torch.manual_seed(71)
    return torch.randint(0, 128, (4, 16)), torch.randint(0, 128, (4, 16))


def _pp_worker(rank, world):
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models.moe_transformer import (
        build_moe_pipeline)
    from easyparallellibrary_amd.ops.distributed_losses import (
        ParallelCrossEntropy)
    epl.init(epl.Config({"cluster.colocate_split_and_replicate": True,
                         "pipeline.num_micro_batch": PP_MICRO}))
    torch.manual_seed(70)
    model = build_moe_pipeline(stages=2, ep=1, **PP_KW)
    engine = epl.Engine(model, loss_fn=ParallelCrossEntropy(),
                        optimizer="adamw", lr=1e-3)
    ids, tgt = _pp_data()
    loss = engine.train_step(ids, tgt)
    gate = model.stages[rank].blocks[0].moe.gate.weight
    return (None if loss is None else float(loss),
            gate.grad.detach().clone())


def _serial_worker(rank, world):
    """the same model run stage after stage in one process by plain
    autograd, micro-batch by micro-batch"""
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models.moe_transformer import (
        build_moe_pipeline)
    from easyparallellibrary_amd.ops.distributed_losses import (
        ParallelCrossEntropy)
    epl.init(epl.Config({"cluster.colocate_split_and_replicate": True}))
    torch.manual_seed(70)
    model = build_moe_pipeline(stages=2, ep=1, **PP_KW)
    loss_fn = ParallelCrossEntropy()
    ids, tgt = _pp_data()
    losses = []
    for i, t in zip(torch.chunk(ids, PP_MICRO), torch.chunk(tgt, PP_MICRO)):
        loss = loss_fn(model(i), t)
        loss.backward()
        losses.append(float(loss.detach()))
    gates = [model.stages[s].blocks[0].moe.gate.weight for s in (0, 1)]
    # the same run without the aux losses, to show they matter
    plain_kw = dict(PP_KW, aux_loss_coef=0.0, z_loss_coef=0.0)
    torch.manual_seed(70)
    plain = build_moe_pipeline(stages=2, ep=1, **plain_kw)
    for i, t in zip(torch.chunk(ids, PP_MICRO), torch.chunk(tgt, PP_MICRO)):
        loss_fn(plain(i), t).backward()
    return (sum(losses) / PP_MICRO,
            [g.grad.detach().clone() for g in gates],
            plain.stages[0].blocks[0].moe.gate.weight.grad.detach().clone())


def test_pp2_gate_gradients_equal_serial():
    """the aux losses of a MoE layer on stage 0 reach its gate although
    the loss lives on the last stage"""
    loss_s, gates_s, plain0 = run_multiprocess(_serial_worker, world=1)[0]
    (loss0, gate0), (loss1, gate1) = run_multiprocess(_pp_worker, world=2)
    assert loss0 is None
    assert abs(loss1 - loss_s) < 1e-5        # the task loss, no aux in it
    # the engine leaves the sum over micro-batches in .grad
    for got, want in ((gate0, gates_s[0]), (gate1, gates_s[1])):
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-7), (
            (got - want).abs().max())
    assert not torch.allclose(gate0, plain0, rtol=1e-2, atol=1e-7)


# ---- what the feature is for ---------------------------------------------------
def _train(coef, steps=100):
    """hidden 32, 8 experts, top-2, 256 tokens of |randn|, a gate skewed
    towards experts 0 and 1, SGD lr 0.5"""
    torch.manual_seed(0)
    layer = ExpertParallelMLP(32, 64, 8, top_k=2, aux_loss_coef=coef)
    with torch.no_grad():
        layer.gate.weight[0] += 0.06
        layer.gate.weight[1] += 0.04
    x = torch.randn(256, 32).abs()
    tgt = torch.randn(256, 32)
    opt = torch.optim.SGD(layer.parameters(), lr=0.5)
    history = []
    for _ in range(steps):
        with torch.no_grad():
            history.append(float(_explicit_aux(layer, x)[0]))
        opt.zero_grad()
        loss = ((layer(x) - tgt) ** 2).mean()
        loss.backward()
        opt.step()
    with torch.no_grad():
        history.append(float(_explicit_aux(layer, x)[0]))
    return history


def test_balance_loss_balances():
    """coefficient 0.1 (1.0 collapses at this learning rate): L_bal ends
    below its start and below the coefficient-0 run's"""
    with_aux = _train(0.1)
    without = _train(0.0)
    print("L_bal with coefficient 0.1: %.3f -> %.3f; with 0: %.3f -> %.3f"
          % (with_aux[0], with_aux[-1], without[0], without[-1]))
    assert with_aux[0] == without[0]
    assert with_aux[0] > 1.5                 # the start is skewed
    assert with_aux[-1] < with_aux[0] - 0.2
    assert with_aux[-1] < without[-1] - 0.2
