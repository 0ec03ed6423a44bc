"""Interval attention (bidirectional packed documents, symmetric windows),
the parts that run without a GPU: interval_bounds against a brute-force
double loop, the torch fallback of interval_attention against the fp64
reference of kernel_refs.py under the brute-force mask, and document
isolation plus the position restart through a packed bert-tiny.  The
contract is the module docstring of ops/attention.py."""

import pytest
import torch

from easyparallellibrary_amd.ops.attention import (
    interval_attention, interval_bounds)
from tests import kernel_refs as kr
from tests.test_attention_band_cpu import CUTS_A, CUTS_B, doc_ids

F64 = torch.float64


def interval_valid(segment_ids, window, seq, lens=None, b=1):
    """[B, 1, S, S] bool by the definition: query i < len sees key j < len
    iff every id between them is equal and |i - j| < window; a padded row
    is given its diagonal so that the reference stays finite (its results
    are not compared)"""
    if segment_ids is not None:
        b = segment_ids.shape[0]
    if lens is not None:
        b = len(lens)
    valid = torch.zeros(b, 1, seq, seq, dtype=torch.bool)
    for n in range(b):
        ids = None if segment_ids is None else segment_ids[n].tolist()
        ln = seq if lens is None else lens[n]
        for i in range(seq):
            valid[n, 0, i, i] = True
            for step in (-1, 1):
                j = i + step
                while i < ln and 0 <= j < ln \
                        and (ids is None or ids[j] == ids[j - step]) \
                        and (window is None or abs(i - j) < window):
                    valid[n, 0, i, j] = True
                    j += step
    return valid


@pytest.mark.parametrize("cuts,window", [
    ((CUTS_A, CUTS_B), None), (None, 1), (None, 70),
    ((CUTS_A, CUTS_B), 70), (None, None)])
def test_interval_bounds_brute_force(cuts, window):
    seq = 300
    ids = None if cuts is None else torch.stack(
        [doc_ids(seq, c) for c in cuts])
    bounds = interval_bounds(ids, window, seq, "cpu")
    rows = 1 if ids is None else 2
    for t in bounds:
        assert t.dtype == torch.int32 and t.is_contiguous()
        assert tuple(t.shape) == (rows, seq)
        assert bool((t[:, 1:] >= t[:, :-1]).all())      # monotone
    kv_lo, kv_hi, q_lo, q_hi = bounds
    pos = torch.arange(seq)
    assert bool((kv_lo <= pos).all()) and bool((pos < kv_hi).all())
    assert bool((q_lo <= pos).all()) and bool((pos < q_hi).all())
    valid = interval_valid(ids, window, seq, b=rows)[:, 0]
    for n in range(rows):
        for lo, hi, m in ((kv_lo, kv_hi, valid[n]), (q_lo, q_hi, valid[n].T)):
            want = (pos >= lo[n, :, None]) & (pos < hi[n, :, None])
            assert torch.equal(m, want)


@pytest.mark.parametrize("hkv", [2, 1])
def test_fallback_matches_fp64_reference(hkv):
    seq, d, window, lens = 72, 32, 20, [50, 72]
    ids = torch.stack([doc_ids(seq, (1, 33)), doc_ids(seq, (31, 32, 64))])
    q, _, _, dout = kr.attn_inputs("randn", seq, d, False, seed=0, b=2, h=2)
    _, k, v, _ = kr.attn_inputs("randn", seq, d, False, seed=1, b=2, h=hkv)
    ke, ve = (t.repeat_interleave(2 // hkv, dim=1) for t in (k, v))
    ref = kr.attn_ref(q, ke, ve, dout, False, d ** -0.5,
                      valid=interval_valid(ids, window, seq, lens))
    for name in ("dk", "dv"):
        ref[name] = ref[name].view(2, hkv, 2 // hkv, seq, d).sum(2)
    tq, tk, tv = (t.clone().requires_grad_() for t in (q, k, v))
    out = interval_attention(
        tq, tk, tv, interval_bounds(ids, window, seq, "cpu"),
        seqlens=torch.tensor(lens, dtype=torch.int32))
    out.backward(dout)
    got = dict(out=out.detach(), dq=tq.grad, dk=tk.grad, dv=tv.grad)
    for name, t in got.items():
        for n, ln in enumerate(lens):
            assert not bool(t[n, :, ln:].abs().any()), name
            torch.testing.assert_close(t[n, :, :ln], ref[name][n, :, :ln],
                                       rtol=1e-9, atol=1e-9)


def test_bert_documents_are_isolated_and_positions_restart():
    from easyparallellibrary_amd.models.bert import build_bert
    torch.manual_seed(0)
    model = build_bert("bert-tiny", vocab_size=64, max_pos=96).double()
    seq, cut = 96, 40
    seg = doc_ids(seq, (cut,))[None].expand(2, seq)
    ids = torch.randint(0, 64, (2, seq))
    other = ids.clone()
    other[:, :cut] = (ids[:, :cut] + 1) % 64
    with torch.no_grad():
        a, b = model(ids, segment_ids=seg), model(other, segment_ids=seg)
        leaky = model(other)
        alone = model(ids[:, cut:])
    assert torch.equal(a[:, cut:], b[:, cut:])
    assert not torch.equal(a[:, :cut], b[:, :cut])
    assert not torch.equal(a[:, cut:], leaky[:, cut:])
    # document 1 alone in a row of its own length: the same attention and,
    # only if its positions restarted at 0, the same embeddings.  The two
    # runs reduce over rows of different lengths, hence no bit equality.
    torch.testing.assert_close(a[:, cut:], alone, rtol=1e-9, atol=1e-9)
    with pytest.raises(NotImplementedError):
        build_bert("bert-tiny", vocab_size=64, max_pos=96, num_stages=2)(
            ids, segment_ids=seg)
