"""ExpertParallelMLP with the load-balance and z losses on the GPU: the
fused router (csrc/kernels/moe_router.hip) against the torch path of the
same semantics on the same device, and a hipGraph-captured step against
the eager one."""

import pytest
import torch

pytestmark = pytest.mark.gpu

C_BAL, C_Z = 0.1, 0.01
U_BF16 = 2.0 ** -8


def _close(got, ref, name):
    """2^-8 of the element's magnitude plus 2^-8 of the tensor's RMS: an
    element is a sum of n addends of some size s, of magnitude about
    s sqrt(n), and each path rounds addends of summed magnitude s n to
    bf16; the RMS stands in for that sum where the terms cancel."""
    got, ref = got.float(), ref.float()
    tol = U_BF16 * (got.abs() + ref.abs()) + U_BF16 * ref.pow(2).mean().sqrt()
    err = (got - ref).abs()
    assert bool((err <= tol).all()), (name, float((err / tol).max()))
    return float((err / tol).max())


@pytest.mark.parametrize("experts", [8, 24])
def test_fused_router_matches_torch_path(experts):
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.ops.moe import ExpertParallelMLP
    epl.init()
    tokens, hidden = 64, 64

    def build(fused):
        torch.manual_seed(10)
        return ExpertParallelMLP(
            hidden, 128, experts, top_k=2, aux_loss_coef=C_BAL,
            z_loss_coef=C_Z, fused_router=fused).to("cuda", torch.bfloat16)

    torch.manual_seed(11)
    x0 = torch.randn(tokens, hidden, device="cuda", dtype=torch.bfloat16)
    # the gate copies the first ``experts`` columns of x (one exact product
    # per logit), and those hold a permutation of distinct multiples of
    # 0.25 per token: no two logits of a row are equal, on any GEMM
    perm = torch.rand(tokens, experts, device="cuda").argsort(dim=1)
    x0[:, :experts] = (perm.float() * 0.25 - experts * 0.125).to(
        torch.bfloat16)
    tgt = torch.randn(tokens, hidden, device="cuda", dtype=torch.bfloat16)
    res = {}
    for fused in (True, False):
        m = build(fused)
        with torch.no_grad():
            m.gate.weight.zero_()
            m.gate.weight[:, :experts] = torch.eye(
                experts, device="cuda", dtype=torch.bfloat16)
        x = x0.clone().requires_grad_(True)
        assert m._router_mode(x) == ("fused" if fused else "torch")
        with torch.no_grad():
            logits = m.gate(x)
            top3 = logits.float().topk(3, dim=-1).values
            # no ties among the three largest: both paths have to agree
            assert bool(((top3[:, 0] > top3[:, 1]) &
                         (top3[:, 1] > top3[:, 2])).all())
            topi = m._route(x, m._router_mode(x))[0]
        out = m(x)
        (out.float() * tgt.float()).sum().backward()
        torch.cuda.synchronize()
        res[fused] = dict(
            topi=topi, out=out.detach(), x=x.grad,
            counts=m.last_expert_counts.clone(),
            bal=m.last_balance_loss.float().clone(),
            z=m.last_z_loss.float().clone(),
            **{n: p.grad for n, p in m.named_parameters()})
    f, t = res[True], res[False]
    assert torch.equal(f["topi"], t["topi"])
    assert torch.equal(f["counts"], t["counts"])
    assert torch.allclose(f["bal"], t["bal"], rtol=1e-5)
    assert torch.allclose(f["z"], t["z"], rtol=1e-5)
    worst = {n: _close(f[n], t[n], n)
             for n in ("out", "x", "gate.weight", "w1", "w2")}
    print("E %d fused vs torch, worst err / tol: %s" % (
        experts, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def _arena_grad(engine, param):
    """the step's gradient of ``param``: the engine keeps gradients in its
    flat arenas (a captured step never touches ``param.grad``)"""
    for group in engine.flat_groups:
        try:
            return group.arena_view_of(param).float().clone()
        except KeyError:
            continue
    raise KeyError("parameter in no flat group")


def _engine_run(graphed, steps=4):
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models.moe_transformer import (
        build_moe_transformer)
    from easyparallellibrary_amd.ops.distributed_losses import (
        ParallelCrossEntropy)
    from easyparallellibrary_amd.ops.moe import moe_aux_losses

    epl.init(epl.Config({"kernel.hip_graph": graphed,
                         "cluster.colocate_split_and_replicate": True}))
    torch.manual_seed(5)
    model = build_moe_transformer(world=1, layers=2, hidden=128, heads=2,
                                  ffn=256, num_experts=4, vocab_size=512,
                                  max_pos=64, aux_loss_coef=C_BAL,
                                  z_loss_coef=C_Z)
    engine = epl.Engine(model, loss_fn=ParallelCrossEntropy(),
                        optimizer="adamw", lr=1e-3, dtype=torch.bfloat16)
    torch.manual_seed(11)
    ids = torch.randint(0, 512, (4, 64), device=engine.device)
    tgt = torch.randint(0, 512, (4, 64), device=engine.device)
    losses, aux = [], []
    for _ in range(steps):
        losses.append(float(engine.train_step(ids, tgt)))
        a = moe_aux_losses(model)
        aux.append((float(a["balance_loss"]), float(a["z_loss"])))
    torch.cuda.synchronize()
    moe = model.blocks[0].moe
    probe = torch.zeros(1, 128, device=engine.device, dtype=torch.bfloat16)
    assert moe._router_mode(probe) == "fused"
    return engine, losses, aux, _arena_grad(engine, moe.gate.weight)


def test_hipgraph_step_with_aux_losses_matches_eager():
    from easyparallellibrary_amd.runtime.hipgraph import HipGraphStep
    engine_g, losses_g, aux_g, gate_g = _engine_run(True)
    assert isinstance(engine_g._hipgraph, HipGraphStep)
    assert engine_g._hipgraph.graph is not None
    engine_e, losses_e, aux_e, gate_e = _engine_run(False)
    assert engine_e._hipgraph is False
    for lg, le in zip(losses_g, losses_e):
        assert abs(lg - le) <= 0.05 * abs(le) + 1e-2, (losses_g, losses_e)
    for (bg, zg), (be, ze) in zip(aux_g, aux_e):
        assert abs(bg - be) <= 0.05 * abs(be) + 1e-2, (aux_g, aux_e)
        assert abs(zg - ze) <= 0.05 * abs(ze) + 1e-2, (aux_g, aux_e)
    # the aux losses of the replayed steps are those steps' own
    assert len({a for a in aux_g}) > 1
    rel = (gate_g - gate_e).norm() / gate_e.norm()
    assert float(rel) <= 0.05, float(rel)
    assert float(gate_e.norm()) > 0
