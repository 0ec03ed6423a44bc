"""The live-row kernels (rows_live_index, gather_rows, scatter_rows_zero)
exactly against torch constructions, and LiveRowsLinear on the device
against the fp64 product of the same inputs.  Shapes, masks and the GEMM
bound: tests/lm_head_cases.py.  Every test prints its worst err / E."""

import pytest
import torch

import easyparallellibrary_amd as epl
from easyparallellibrary_amd.models import bert, gpt2
from easyparallellibrary_amd.ops import lm_head as lh
from tests import kernel_refs as kr
from tests import lm_head_cases as lc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from easyparallellibrary_amd import _C
else:
    _C = None

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = {"bf16": BF16, "f32": F32}


def dev():
    return torch.device("cuda:0")


def check_index(g, live):
    """rows_live_index against the mask, and against torch's own != 0"""
    n = g.shape[0]
    idx, count, inv = _C.rows_live_index(g)
    want = live.nonzero().squeeze(1).to(torch.int32)
    assert torch.equal((g != 0).any(dim=1).cpu(), live)
    assert idx.dtype == inv.dtype == count.dtype == torch.int32
    assert idx.shape == (n,) and inv.shape == (n,) and count.shape == (1,)
    c = int(count)
    assert c == want.numel()
    idx_c, inv_c = idx.cpu(), inv.cpu()
    assert torch.equal(idx_c[:c], want)
    if c > 1:
        assert bool((idx_c[1:c] > idx_c[:c - 1]).all())   # ascending
    assert bool((idx_c[c:] == -1).all())
    want_inv = torch.full((n,), -1, dtype=torch.int32)
    want_inv[want.long()] = torch.arange(c, dtype=torch.int32)
    assert torch.equal(inv_c, want_inv)
    return idx, count, inv, want.long()


@pytest.mark.parametrize("dt", ("bf16", "f32"))
@pytest.mark.parametrize("mask", lc.MASKS)
@pytest.mark.parametrize("v", lc.VS)
@pytest.mark.parametrize("n", lc.NS)
def test_kernels_exact(n, v, mask, dt):
    dtype = DTYPES[dt]
    g_cpu, live = lc.grad_matrix(mask, n, v, dtype)
    g = g_cpu.to(dev())
    idx, count, inv, want = check_index(g, live)
    c = want.numel()
    # pad rows exist unless c is a multiple of 256 (0 and 256 among the
    # cases); one more row than the pad at the exact multiples
    n_pad = lh.pad_rows(c) if c % 256 else c + 1
    nan = float("nan")
    out = torch.full((n_pad, v), nan, dtype=dtype, device=dev())
    g_c = _C.gather_rows(g, idx, count, n_pad, out=out)
    assert g_c.data_ptr() == out.data_ptr()
    exp = torch.zeros(n_pad, v, dtype=dtype)
    exp[:c] = g_cpu[want]
    assert torch.equal(lc.bits(g_c.cpu()), lc.bits(exp))
    fresh = _C.gather_rows(g, idx, count, n_pad)
    assert torch.equal(lc.bits(fresh.cpu()), lc.bits(exp))

    src_cpu = torch.randn(n_pad, lc.H).to(dtype)
    src_cpu[c:] = 7.0        # pad rows of the source must not be copied
    buf = torch.full((n, lc.H), nan, dtype=dtype, device=dev())
    sc = _C.scatter_rows_zero(src_cpu.to(dev()), inv, out=buf)
    assert sc.data_ptr() == buf.data_ptr()
    exp = torch.zeros(n, lc.H, dtype=dtype)
    exp[want] = src_cpu[:c]
    assert not bool(torch.isnan(sc).any())
    assert torch.equal(lc.bits(sc.cpu()), lc.bits(exp))
    # a second run gives the same bits
    idx2, count2, inv2 = _C.rows_live_index(g)
    assert torch.equal(idx, idx2) and torch.equal(inv, inv2)
    assert torch.equal(count, count2)


def test_special_rows_are_in_the_mixed_case():
    g, live = lc.grad_matrix("mixed", 1000, 1000, BF16)
    assert bool(live[1]) and int((g[1] != 0).sum()) == 1 and g[1, -1] != 0
    assert not bool(live[2]) and bool((lc.bits(g[2]) == -32768).all())
    assert bool(live[5]) and int(torch.isnan(g[5]).sum()) == 1
    assert bool(live[255]) and not bool(live[256]) and bool(live[257])


def test_bindings_refuse_what_the_kernels_cannot_take():
    g = torch.zeros(16, 8, dtype=BF16, device=dev())
    idx, count, inv = _C.rows_live_index(g)
    with pytest.raises(RuntimeError):
        _C.rows_live_index(torch.zeros(16, 12, dtype=BF16, device=dev()))
    with pytest.raises(RuntimeError):
        _C.rows_live_index(g.t())
    with pytest.raises(RuntimeError):
        _C.rows_live_index(g.half())
    with pytest.raises(RuntimeError):
        _C.gather_rows(g, idx[:8], count, 16)
    with pytest.raises(RuntimeError):
        _C.gather_rows(g, idx, count, 0)
    with pytest.raises(RuntimeError):
        _C.gather_rows(g, idx, count, 16, out=torch.empty(
            8, 8, dtype=BF16, device=dev()))
    with pytest.raises(RuntimeError):
        _C.scatter_rows_zero(g, inv.long())


# ---- the Function --------------------------------------------------------------
def run_function(x, w, g):
    xa = x.clone().requires_grad_(True)
    wa = w.clone().requires_grad_(True)
    lh.LiveRowsLinear.apply(xa, wa).backward(g)
    torch.cuda.synchronize()
    return xa.grad, wa.grad


def judge(tag, dx, dw, refs, factor):
    worst = {}
    for name, got in (("dx", dx), ("dw", dw)):
        worst[name] = kr.ratio_of(got.to(lc.F64).cpu(), refs[name],
                                  refs["e_" + name])
    print("{}: worst err / E dx {:.3f} dw {:.3f} (allowed {})".format(
        tag, worst["dx"], worst["dw"], factor))
    assert worst["dx"] <= factor and worst["dw"] <= factor, worst


@pytest.mark.parametrize("path,dt", (("live", "bf16"), ("live", "f32"),
                                     ("auto", "bf16"), ("dense", "bf16")))
@pytest.mark.parametrize("mask", lc.MASKS)
@pytest.mark.parametrize("v", lc.VS)
@pytest.mark.parametrize("n", lc.NS)
def test_function_inside_gemm_bound(n, v, mask, path, dt, monkeypatch):
    """live: break-even lifted, the compact GEMMs run at every N (n_pad
    exceeds N at the small ones); auto: as shipped; dense: the dense
    GEMMs.  All three inside the same bound."""
    dtype = DTYPES[dt]
    calls = []
    real = lh.live_rows_backward

    def spy(*a):
        out = real(*a)
        calls.append((a[3], out is not None))
        return out

    monkeypatch.setattr(lh, "live_rows_backward", spy)
    if path == "live":
        monkeypatch.setattr(lh, "DENSE_FRACTION", 1e9)
    elif path == "dense":
        monkeypatch.setattr(lh, "live_rows_mode", lambda *a: None)
    x, w = (t.to(dev()) for t in lc.head_inputs(n, v, dtype))
    g_cpu, live = lc.grad_matrix(mask, n, v, dtype, specials=False)
    g = g_cpu.to(dev())
    dx, dw = run_function(x, w, g)
    n_pad = lh.pad_rows(int(live.sum()))
    compact = path == "live" or (path == "auto" and n_pad < 0.5 * n)
    assert calls == ([] if path == "dense" else [("native", compact)])
    assert dx.shape == x.shape and dw.shape == w.shape
    assert dx.dtype == dtype and dw.dtype == dtype
    refs = lc.head_refs(x, w, g, bf16=dtype == BF16)
    judge("n{} v{} {} {} {}".format(n, v, mask, dt, path), dx, dw, refs,
          2.0 if dtype == BF16 else 1.0)
    if compact:
        # dead rows of dX are exactly +0, and two runs agree bit for bit
        assert bool((lc.bits(dx.cpu())[~live] == 0).all())
        dx2, dw2 = run_function(x, w, g)
        assert torch.equal(lc.bits(dx), lc.bits(dx2))
        assert torch.equal(lc.bits(dw), lc.bits(dw2))


def test_count_zero_runs_no_gemm(monkeypatch):
    x, w = (t.to(dev()) for t in lc.head_inputs(1000, 1032, BF16))
    g = torch.zeros(1000, 1032, dtype=BF16, device=dev())
    g[17] = -0.0

    def no_gemm(*a, **k):
        raise AssertionError("a GEMM operand was built")

    monkeypatch.setattr(lh, "dense_backward", no_gemm)
    monkeypatch.setattr(lh, "gather_rows", no_gemm)
    dx, dw = run_function(x, w, g)
    assert dx.shape == x.shape and dw.shape == w.shape
    assert bool((lc.bits(dx) == 0).all()) and bool((lc.bits(dw) == 0).all())


def test_forward_keeps_the_linear_bits_and_3d_shapes():
    x, w = (t.to(dev()) for t in lc.head_inputs(1000, 1032, BF16))
    x3 = x.reshape(4, 250, lc.H).requires_grad_(True)
    wa = w.clone().requires_grad_(True)
    y = lh.LiveRowsLinear.apply(x3, wa)
    assert torch.equal(y, torch.nn.functional.linear(x3, w))
    g, _ = lc.grad_matrix("mixed", 1000, 1032, BF16, specials=False)
    y.backward(g.to(dev()).reshape(4, 250, 1032))
    assert x3.grad.shape == x3.shape and wa.grad.shape == w.shape
    # a gradient that is a non-contiguous view runs dense
    assert lh.live_rows_mode(g.to(dev())[:, ::2], x, w) is None
    assert lh.live_rows_mode(g.to(dev()), x, w) == "native"


def test_capturing_stream_runs_dense():
    x, w = (t.to(dev()) for t in lc.head_inputs(1000, 1032, BF16))
    g, _ = lc.grad_matrix("mixed", 1000, 1032, BF16, specials=False)
    g = g.to(dev())
    seen = []
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        out = torch.empty(8, device=dev())
        with torch.cuda.graph(graph, stream=s):
            seen.append(lh.live_rows_mode(g, x, w))
            out.fill_(1.0)
    torch.cuda.synchronize()
    assert seen == [None]


def _mlm_step(model, vocab, batch=8, seq=128):
    ids, tgt = bert.synthetic_mlm_batch(batch, seq, vocab, device=dev(),
                                        seed=3)
    logits = model(ids)
    loss = torch.nn.functional.cross_entropy(
        logits.reshape(-1, vocab).float(), tgt.reshape(-1),
        ignore_index=-100)
    loss.backward()
    torch.cuda.synchronize()


def test_bert_head_takes_the_live_row_path_gpt2_does_not(monkeypatch):
    monkeypatch.delenv("EPL_LMHEAD_LIVE_ROWS", raising=False)
    epl.init()
    calls = []
    real = lh.live_rows_backward

    def spy(*a):
        out = real(*a)
        calls.append((a[3], out is not None, tuple(a[0].shape)))
        return out

    monkeypatch.setattr(lh, "live_rows_backward", spy)
    vocab = 512
    model = bert.build_bert("bert-tiny", vocab_size=vocab,
                            max_pos=128).to(dev(), dtype=BF16)
    _mlm_step(model, vocab)
    assert calls == [("native", True, (8 * 128, vocab))]
    assert bool(torch.isfinite(model.head.proj.weight.grad).all())
    del calls[:]
    gpt = gpt2.build_gpt2("gpt2-tiny", vocab_size=vocab,
                          max_pos=128).to(dev(), dtype=BF16)
    _mlm_step(gpt, vocab)
    assert calls == []
