"""Interval flash attention (csrc/kernels/attention_interval.hip): direct
_C.attn_fwd_interval / _C.attn_bwd_interval calls against the fp64
reference of kernel_refs.py under the brute-force mask of
test_attention_interval_cpu.py, |got - ref| <= ATTN_FACTOR x the derived
bound of attn_bounds (dk / dv and their bounds summed over each group), as
test_attention_band_gpu.py judges.

The cases reach every phase: documents with a length-1 document, a
boundary on the 128 edge and around the 32 / 64 edges, a tail document over
more than one block (block 2: a head tile and two bulk tiles; block 1: no
bulk phase); window 200 (block 1: head, four bulk tiles, tail); windows
1 / 32 / 33 / 100 at an odd length; prefix-LM bounds written directly
(hidden keys after a row's visible ones); documents + window + seqlens.
The two samples of a batch are bounded differently."""

import functools

import pytest
import torch

from tests import attn_group_cases as gc
from tests import kernel_refs as kr
from tests.test_attention_band_cpu import CUTS_A, CUTS_B, doc_ids
from tests.test_attention_interval_cpu import interval_valid

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16
B = 2
# name -> (seq, document cuts per sample or None, window, seqlens)
CASES = {
    "docs": (384, (CUTS_A, CUTS_B), None, None),
    "win200": (384, None, 200, None),
    "win1": (257, None, 1, None),
    "win32": (257, None, 32, None),
    "win33": (257, None, 33, None),
    "win100": (257, None, 100, None),
    "prefix_lm": (384, None, None, None),
    "docs_win70_lens": (384, (CUTS_A, CUTS_B), 70, [300, 129]),
}
PREFIX = (70, 200)


def prefix_lm(seq):
    """(kv_lo, kv_hi, q_lo, q_hi), int64 [B, S], of the prefix-LM case"""
    pos = torch.arange(seq)
    p = torch.tensor(PREFIX)[:, None]
    kv_hi = torch.maximum(pos + 1, p)
    q_lo = torch.where(pos < p, 0, pos)
    return (torch.zeros(B, seq, dtype=torch.int64), kv_hi, q_lo,
            torch.full((B, seq), seq))


@functools.lru_cache(maxsize=None)
def mask_of(name):
    """(seq, lens, [B, 1, S, S] mask) of a case; needs no GPU.  Shared:
    nobody writes into the mask"""
    seq, cuts, window, lens = CASES[name]
    if name == "prefix_lm":
        kv_hi = prefix_lm(seq)[1]
        pos = torch.arange(seq)
        return seq, lens, (pos[None, None, :] < kv_hi[:, :, None])[:, None]
    ids = None if cuts is None else torch.stack(
        [doc_ids(seq, c) for c in cuts])
    return seq, lens, interval_valid(ids, window, seq, lens or [seq] * B)


def case_of(name):
    """(seq, lens, device bounds, [B, 1, S, S] mask) of a case"""
    from easyparallellibrary_amd.ops.attention import interval_bounds
    seq, lens, valid = mask_of(name)
    if name == "prefix_lm":
        bounds = tuple(t.int().contiguous().cuda() for t in prefix_lm(seq))
        return seq, lens, bounds, valid
    _, cuts, window, _ = CASES[name]
    ids = None if cuts is None else torch.stack(
        [doc_ids(seq, c) for c in cuts])
    bounds = interval_bounds(None if ids is None else ids.cuda(), window,
                             seq, "cuda")
    return seq, lens, bounds, valid


def inputs(family, seq, d, h, hkv, valid=None, lens=None):
    """the joint families of attn_group_cases.py under the case's mask
    (None: randn, which needs none)"""
    assert valid is not None or family == "randn"
    return gc.group_inputs(family, seq, d, h, hkv, B, valid, lens=lens)


reference = gc.group_reference


def run(q, k, v, dout, bounds, lens=None):
    """one forward + backward through the bindings; results on the CPU.
    bounds None: today's non-causal kernels (MHA or GQA) instead"""
    from easyparallellibrary_amd import _C
    b, h, seq, d = q.shape
    tq, tk, tv, tdo = (t.to(BF16).cuda() for t in (q, k, v, dout))
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (tq, tk, tv))
    out = torch.full((b, seq, h, d), float("nan"), dtype=BF16,
                     device="cuda").permute(0, 2, 1, 3)
    lse = torch.full((b * h * seq,), float("nan"), device="cuda")
    delta = torch.full_like(lse, float("nan"))
    sl = None if lens is None else torch.tensor(lens, dtype=torch.int32,
                                                device="cuda")
    scale = d ** -0.5
    if bounds is not None:
        _C.attn_fwd_interval(tq, tk, tv, out, lse, scale, *bounds[:2], sl)
        _C.attn_bwd_interval(tq, tk, tv, out, tdo, lse, delta, dq, dk, dv,
                             scale, *bounds, sl)
    elif k.shape[1] == h:
        _C.attn_fwd(tq, tk, tv, out, lse, scale, False, None, 0, 0, 1.0, sl)
        _C.attn_bwd(tq, tk, tv, out, tdo, lse, delta, dq, dk, dv, scale,
                    False, True, None, 1.0, None, sl)
    else:
        _C.attn_fwd_gqa(tq, tk, tv, out, lse, scale, False, sl)
        _C.attn_bwd_gqa(tq, tk, tv, out, tdo, lse, delta, dq, dk, dv, scale,
                        False, sl)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu(),
                lse=lse.cpu().view(b, h, seq))


def check(got, ref, bounds, lens, tag):
    """every output finite; inside its bound on the valid rows and an
    exact zero on the padded ones"""
    for name, t in got.items():
        t = t.to(F64)
        assert bool(torch.isfinite(t).all()), name
        for n in range(t.shape[0]):
            ln = t.shape[2] if lens is None else lens[n]
            assert not bool(t[n, :, ln:].abs().any()), name
            ratio = kr.attn_ratio(
                (t[n, :, :ln] - ref[name][n, :, :ln]).abs(),
                bounds[name][n, :, :ln])
            print("INTERVAL-RATIO {} {} {:.3f}".format(tag, name, ratio))
            assert ratio <= kr.ATTN_FACTOR[name], (name, n, ratio)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("family", kr.ATTN_FAMILIES)
@pytest.mark.parametrize("h,hkv", [(4, 4), (4, 2)])
@pytest.mark.parametrize("d", [64, 128])
def test_interval_against_fp64(d, h, hkv, family, case):
    seq, lens, bounds, valid = case_of(case)
    inp = inputs(family, seq, d, h, hkv, valid, lens)
    ref, limits = reference(*inp, valid)
    check(run(*inp, bounds, lens), ref, limits, lens, "plain")


@pytest.mark.parametrize("case", ["docs", "docs_win70_lens"])
@pytest.mark.parametrize("family", kr.ATTN_FAMILIES)
@pytest.mark.parametrize("d", [64, 128])
def test_qkv_interval_attention_against_fp64(d, family, case):
    """the packed [B, S, 3, H, D] buffer; gradients from the one d_qkv"""
    from easyparallellibrary_amd.ops.attention import qkv_interval_attention
    seq, lens, bounds, valid = case_of(case)
    q, k, v, dout = inputs(family, seq, d, 4, 4, valid, lens)
    ref, limits = reference(q, k, v, dout, valid)
    qkv = torch.stack([t.transpose(1, 2) for t in (q, k, v)], 2).to(
        BF16).cuda().requires_grad_()
    sl = None if lens is None else torch.tensor(lens, dtype=torch.int32,
                                                device="cuda")
    out = qkv_interval_attention(qkv, bounds, seqlens=sl)
    out.backward(dout.to(BF16).cuda())
    gq, gk, gv = (qkv.grad[:, :, i].transpose(1, 2).cpu() for i in range(3))
    check(dict(out=out.detach().cpu(), dq=gq, dk=gk, dv=gv), ref, limits,
          lens, "packed")


@pytest.mark.parametrize("lens", [None, [130, 77]])
@pytest.mark.parametrize("seq", [200, 384])
@pytest.mark.parametrize("h,hkv", [(4, 4), (4, 2)])
@pytest.mark.parametrize("d", [64, 128])
def test_trivial_interval_gives_the_non_causal_bits(d, h, hkv, seq, lens):
    """bounds 0 and S everywhere: the head phase is empty, the tile order
    and the bodies are the non-causal kernels', and a masked tile in which
    nothing is masked computes what a plain tile computes"""
    inp = inputs("randn", seq, d, h, hkv)
    want = run(*inp, None, lens)
    zero = torch.zeros(B, seq, dtype=torch.int32, device="cuda")
    full = torch.full_like(zero, seq)
    got = run(*inp, (zero, full, zero, full), lens)
    for name in ("out", "dq", "dk", "dv"):
        assert torch.equal(got[name].view(torch.int16),
                           want[name].view(torch.int16)), name


@pytest.mark.parametrize("bad", [
    dict(kv_lo=384 + 5), dict(kv_hi=0), dict(q_lo=384 + 5), dict(q_hi=0),
    dict(kv_lo=-7, kv_hi=-7, q_lo=-7, q_hi=-7)])
@pytest.mark.parametrize("d", [64, 128])
def test_hostile_bounds_stay_inside_the_buffers(d, bad):
    """bounds the kernels must clamp (lower to [0, i], upper to [i + 1,
    len]): finite results, untouched guard rows; no value is asserted"""
    from easyparallellibrary_amd import _C
    seq, h = 384, 4
    lay = kr.attn_layout("plain", B, h, seq, d, "cuda")
    for name, t in zip(("q", "k", "v", "dout"),
                       inputs("randn", seq, d, h, h)):
        lay[name].copy_(t.to(BF16))
    lse, delta = (kr.attn_flat(B * h * seq, torch.float32, "cuda")
                  for _ in range(2))
    fill = {**dict(kv_lo=0, kv_hi=seq, q_lo=0, q_hi=seq), **bad}
    bounds = [torch.full((B, seq), fill[n], dtype=torch.int32, device="cuda")
              for n in ("kv_lo", "kv_hi", "q_lo", "q_hi")]
    sl = torch.tensor([seq, 201], dtype=torch.int32, device="cuda")
    scale = d ** -0.5
    _C.attn_fwd_interval(lay["q"], lay["k"], lay["v"], lay["out"], lse.view,
                         scale, *bounds[:2], sl)
    _C.attn_bwd_interval(lay["q"], lay["k"], lay["v"], lay["out"],
                         lay["dout"], lse.view, delta.view, lay["dq"],
                         lay["dk"], lay["dv"], scale, *bounds, sl)
    torch.cuda.synchronize()
    for name in ("out", "dq", "dk", "dv"):
        assert bool(torch.isfinite(lay[name].float()).all()), name
    for name, buf in list(lay["buffers"].items()) + [("lse", lse),
                                                     ("delta", delta)]:
        assert buf.stray_writes() == 0, name


@pytest.mark.parametrize("d,hkv", [(64, 4), (128, 2)])
def test_interval_is_deterministic(d, hkv):
    seq, lens, bounds, valid = case_of("docs_win70_lens")
    inp = inputs("peaked", seq, d, 4, hkv, valid, lens)
    a, b = run(*inp, bounds, lens), run(*inp, bounds, lens)
    for name in a:
        bits = torch.int16 if a[name].dtype == BF16 else torch.int32
        assert torch.equal(a[name].view(bits), b[name].view(bits)), name
