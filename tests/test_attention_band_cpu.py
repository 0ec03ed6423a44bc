"""Banded causal attention (packed documents, sliding windows), the parts
that run without a GPU: band_bounds against a brute-force double loop, the
torch fallback of flash_attention against the fp64 reference of
kernel_refs.py under the brute-force mask, and document isolation through
a llama-tiny-swa model.  The contract is the module docstring of
ops/attention.py."""

import pytest
import torch

from easyparallellibrary_amd.ops.attention import band_bounds, flash_attention
from tests import kernel_refs as kr

F64 = torch.float64


def doc_ids(seq, cuts):
    """[seq] ids of the documents that start at 0 and at every cut.  The
    ids alternate 7, 3, 7, ..: unsorted and repeated, as the contract
    allows."""
    ids = torch.zeros(seq, dtype=torch.int64)
    for c in cuts:
        ids[c:] += 1
    return torch.where(ids % 2 == 0, 7, 3)


def band_valid(segment_ids, window, seq, lens=None):
    """[B, 1, S, S] bool by the definition: query i < len sees key j iff
    both lie in one run of equal ids, i - window < j <= i and j < len; a
    padded row is given its diagonal so that the reference stays finite
    (its results are not compared)"""
    b = 1 if segment_ids is None else segment_ids.shape[0]
    if lens is not None:
        b = len(lens)
    valid = torch.zeros(b, 1, seq, seq, dtype=torch.bool)
    for n in range(b):
        ids = None if segment_ids is None else segment_ids[n].tolist()
        ln = seq if lens is None else lens[n]
        for i in range(seq):
            valid[n, 0, i, i] = True
            for j in range(i - 1, -1, -1):
                if i >= ln or (ids is not None and ids[j] != ids[j + 1]) \
                        or (window is not None and j <= i - window):
                    break
                valid[n, 0, i, j] = True
    return valid


CUTS_A, CUTS_B = (1, 33, 128, 200), (31, 32, 64, 129, 257)


@pytest.mark.parametrize("cuts,window", [
    ((CUTS_A, CUTS_B), None), (None, 1), (None, 70), (None, 1000),
    ((CUTS_A, CUTS_B), 70), (((5,), (6, 7)), 3)])
def test_band_bounds_brute_force(cuts, window):
    seq = 300
    ids = None if cuts is None else torch.stack(
        [doc_ids(seq, c) for c in cuts])
    kv_lo, q_hi = band_bounds(ids, window, seq, "cpu")
    rows = 1 if ids is None else 2
    for t in (kv_lo, q_hi):
        assert t.dtype == torch.int32 and t.is_contiguous()
        assert tuple(t.shape) == (rows, seq)
        assert bool((t[:, 1:] >= t[:, :-1]).all())      # monotone
    pos = torch.arange(seq)
    assert bool((kv_lo <= pos).all()) and bool((pos < q_hi).all())
    valid = band_valid(ids, window, seq)[:, 0]
    for n in range(rows):
        for i in range(seq):
            seen = valid[n, i].nonzero().flatten()
            assert int(kv_lo[n, i]) == int(seen[0]) and int(seen[-1]) == i
            by = valid[n, :, i].nonzero().flatten()
            assert int(by[0]) == i and int(q_hi[n, i]) == int(by[-1]) + 1


@pytest.mark.parametrize("hkv", [2, 1])
def test_fallback_matches_fp64_reference(hkv):
    seq, d, window, lens = 72, 32, 20, [50, 72]
    ids = torch.stack([doc_ids(seq, (1, 33)), doc_ids(seq, (31, 32, 64))])
    q, _, _, dout = kr.attn_inputs("randn", seq, d, True, seed=0, b=2, h=2)
    _, k, v, _ = kr.attn_inputs("randn", seq, d, True, seed=1, b=2, h=hkv)
    ke, ve = (t.repeat_interleave(2 // hkv, dim=1) for t in (k, v))
    ref = kr.attn_ref(q, ke, ve, dout, True, d ** -0.5,
                      valid=band_valid(ids, window, seq, lens))
    for name in ("dk", "dv"):
        ref[name] = ref[name].view(2, hkv, 2 // hkv, seq, d).sum(2)
    tq, tk, tv = (t.clone().requires_grad_() for t in (q, k, v))
    out = flash_attention(tq, tk, tv, causal=True, segment_ids=ids,
                          window=window,
                          seqlens=torch.tensor(lens, dtype=torch.int32))
    out.backward(dout)
    got = dict(out=out.detach(), dq=tq.grad, dk=tk.grad, dv=tv.grad)
    for name, t in got.items():
        for n, ln in enumerate(lens):
            assert not bool(t[n, :, ln:].abs().any()), name
            torch.testing.assert_close(t[n, :, :ln], ref[name][n, :, :ln],
                                       rtol=1e-9, atol=1e-9)


def test_non_causal_band_raises():
    q = torch.zeros(1, 1, 8, 64)
    with pytest.raises(ValueError):
        flash_attention(q, q, q, causal=False, window=4)
    with pytest.raises(ValueError):
        flash_attention(q, q, q, causal=False,
                        segment_ids=torch.zeros(1, 8, dtype=torch.int64))


def test_llama_documents_are_isolated():
    from easyparallellibrary_amd.models.llama import build_llama
    torch.manual_seed(0)
    model = build_llama("llama-tiny-swa", vocab_size=64).double()
    seq, cut = 96, 40
    seg = doc_ids(seq, (cut,))[None].expand(2, seq)
    ids = torch.randint(0, 64, (2, seq))
    other = ids.clone()
    other[:, :cut] = (ids[:, :cut] + 1) % 64
    with torch.no_grad():
        a, b = model(ids, seg), model(other, seg)
        leaky = model(other)
    assert torch.equal(a[:, cut:], b[:, cut:])
    assert not torch.equal(a[:, :cut], b[:, :cut])
    # without segment_ids the window alone lets document 0 leak
    assert not torch.equal(a[:, cut:cut + 8], leaky[:, cut:cut + 8])
