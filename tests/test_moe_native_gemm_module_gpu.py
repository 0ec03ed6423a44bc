"""ExpertParallelMLP(expert_gemm=True): the expert FFN on the grouped GEMM
kernels against the torch.bmm path of the same module, the refusal where
the kernels do not apply, and a captured step whose replay reads the row
counts on the device."""

import pytest
import torch

import easyparallellibrary_amd as epl
from easyparallellibrary_amd.ops.moe import ExpertParallelMLP

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from easyparallellibrary_amd import _C
else:
    _C = None

HIDDEN, FFN, EXPERTS, TOKENS, TOP_K = 128, 256, 8, 512, 2
CAPACITY_FACTOR = 1.0        # capacity = the mean count: some over, some under
GEMMS = ("moe_gemm_nn", "moe_gemm_nt", "moe_gemm_tn")


def build(expert_gemm, hidden=HIDDEN):
    torch.manual_seed(10)
    return ExpertParallelMLP(hidden, FFN, EXPERTS, top_k=TOP_K,
                             capacity_factor=CAPACITY_FACTOR,
                             expert_gemm=expert_gemm).to("cuda",
                                                         torch.bfloat16)


def batch(seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(TOKENS, HIDDEN, device="cuda", dtype=torch.bfloat16,
                       generator=gen)


def step(m, x):
    m.zero_grad(set_to_none=True)
    x.grad = None
    y = m(x)
    y.float().pow(2).mean().backward()
    return y


def gate_counts(m, x):
    """per-expert assignment counts from the gate's own output"""
    with torch.no_grad():
        probs = m.gate(x).float().softmax(-1)
        topi = probs.topk(TOP_K, dim=-1).indices.reshape(-1)
    return torch.bincount(topi, minlength=EXPERTS)


def test_matches_the_bmm_path(monkeypatch):
    epl.init()
    calls = {name: 0 for name in GEMMS + ("bmm",)}

    def spy(owner, attr, key):
        real = getattr(owner, attr)

        def counted(*a, **kw):
            calls[key] += 1
            return real(*a, **kw)
        monkeypatch.setattr(owner, attr, counted)
    for name in GEMMS:
        spy(_C, name, name)
    spy(torch, "bmm", "bmm")

    results = {}
    for native in (True, False):
        m = build(native)
        x = batch(3).requires_grad_(True)
        y = step(m, x)
        if native:
            assert calls["bmm"] == 0, calls
            assert all(calls[name] > 0 for name in GEMMS), calls
            counts = gate_counts(m, x.detach())
            cap = max(1, int(CAPACITY_FACTOR * TOKENS * TOP_K / EXPERTS))
            assert int(counts.max()) > cap > int(counts.min()), \
                (counts.tolist(), cap)
        results[native] = [t.detach().float().clone() for t in (
            y, x.grad, m.gate.weight.grad, m.w1.grad, m.w2.grad)]
    assert calls["bmm"] > 0, calls
    torch.cuda.synchronize()
    names = ("out", "x.grad", "gate.weight.grad", "w1.grad", "w2.grad")
    for name, got, want in zip(names, results[True], results[False]):
        rtol = 3e-2 if name == "gate.weight.grad" else 1e-5
        print(name, float((got - want).abs().max()))
        assert torch.allclose(got, want, atol=3e-2, rtol=rtol), name


def test_expert_gemm_true_raises_where_it_does_not_apply():
    epl.init()
    m = build(True, hidden=72)
    x = torch.randn(TOKENS, 72, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="expert_gemm=True"):
        m(x)


def test_captured_step_reads_rows_at_replay():
    epl.init()
    m = build(True)
    first, second = batch(3), batch(4)
    assert not torch.equal(gate_counts(m, first), gate_counts(m, second))
    xs = first.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(m, xs)
    torch.cuda.current_stream().wait_stream(s)
    m.zero_grad(set_to_none=True)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = m(xs)
        ys.float().pow(2).mean().backward()
    with torch.no_grad():
        xs.copy_(second)
    for _ in range(3):                    # several replays, one result
        graph.replay()
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in (ys, xs.grad, m.w1.grad, m.w2.grad)]
    xe = second.clone().requires_grad_(True)
    ye = step(m, xe)
    torch.cuda.synchronize()
    for name, g, w in zip(("out", "x.grad", "w1.grad", "w2.grad"), got,
                          (ye, xe.grad, m.w1.grad, m.w2.grad)):
        assert torch.equal(g, w), name
