"""Banded causal flash attention (csrc/kernels/attention_band.hip): direct
_C.attn_fwd_band / _C.attn_bwd_band calls against the fp64 reference of
kernel_refs.py under the brute-force mask of test_attention_band_cpu.py,
|got - ref| <= ATTN_FACTOR x the derived bound of attn_bounds (dk / dv and
their bounds summed over each group, as in test_attention_gqa_gpu.py).

The band cases reach every phase of the kernels and every position of a
boundary: a length-1 document, a boundary on a block edge (a block with no
off-diagonal tile), boundaries either side of the 32 / 64 / 128 edges, a
document over more than one block, a window that gives block 2 a head
phase, one bulk tile and the diagonal, windows of 1 / 32 / 33 / 100 at an
odd length, and documents + window + seqlens together.  The two samples
of a batch are segmented differently."""

import functools

import pytest
import torch

from tests import attn_group_cases as gc
from tests import kernel_refs as kr
from tests.test_attention_band_cpu import (
    CUTS_A, CUTS_B, band_valid, doc_ids)

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16
B = 2
# name -> (seq, document cuts per sample or None, window, seqlens)
BANDS = {
    "docs": (384, (CUTS_A, CUTS_B), None, None),
    "win200": (384, None, 200, None),
    "win1": (257, None, 1, None),
    "win32": (257, None, 32, None),
    "win33": (257, None, 33, None),
    "win100": (257, None, 100, None),
    "docs_win70_lens": (384, (CUTS_A, CUTS_B), 70, [300, 129]),
}


def band_of(name):
    seq, cuts, window, lens = BANDS[name]
    ids = None if cuts is None else torch.stack(
        [doc_ids(seq, c) for c in cuts])
    return seq, ids, window, lens


@functools.lru_cache(maxsize=None)
def valid_of(name):
    """the brute-force [B, 1, S, S] mask of a case; shared, nobody writes
    into it"""
    seq, ids, window, lens = band_of(name)
    return band_valid(ids, window, seq, lens or [seq] * B)


def inputs(family, seq, d, h, hkv, valid=None, lens=None):
    """the joint families of attn_group_cases.py under the case's mask
    (None: randn, which needs none)"""
    assert valid is not None or family == "randn"
    return gc.group_inputs(family, seq, d, h, hkv, B, valid, lens=lens)


reference = gc.group_reference


def device_bounds(ids, window, seq):
    from easyparallellibrary_amd.ops.attention import band_bounds
    return band_bounds(None if ids is None else ids.cuda(), window, seq,
                       "cuda")


def run(q, k, v, dout, kv_lo, q_hi, lens=None, causal_call=False):
    """one forward + backward through the bindings; results on the CPU.
    causal_call: today's causal kernels (MHA or GQA) instead of the band"""
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
    if not causal_call:
        _C.attn_fwd_band(tq, tk, tv, out, lse, scale, kv_lo, sl)
        _C.attn_bwd_band(tq, tk, tv, out, tdo, lse, delta, dq, dk, dv, scale,
                         kv_lo, q_hi, sl)
    elif k.shape[1] == h:
        _C.attn_fwd(tq, tk, tv, out, lse, scale, True, None, 0, 0, 1.0, sl)
        _C.attn_bwd(tq, tk, tv, out, tdo, lse, delta, dq, dk, dv, scale,
                    True, True, None, 1.0, None, sl)
    else:
        _C.attn_fwd_gqa(tq, tk, tv, out, lse, scale, True, sl)
        _C.attn_bwd_gqa(tq, tk, tv, out, tdo, lse, delta, dq, dk, dv, scale,
                        True, sl)
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
            print("BAND-RATIO {} {} {:.3f}".format(tag, name, ratio))
            assert ratio <= kr.ATTN_FACTOR[name], (name, n, ratio)


@pytest.mark.parametrize("band", list(BANDS))
@pytest.mark.parametrize("family", kr.ATTN_FAMILIES)
@pytest.mark.parametrize("h,hkv", [(4, 4), (4, 2)])
@pytest.mark.parametrize("d", [64, 128])
def test_band_against_fp64(d, h, hkv, family, band):
    seq, ids, window, lens = band_of(band)
    valid = valid_of(band)
    inp = inputs(family, seq, d, h, hkv, valid, lens)
    ref, bounds = reference(*inp, valid)
    got = run(*inp, *device_bounds(ids, window, seq), lens)
    check(got, ref, bounds, lens, "plain")


@pytest.mark.parametrize("band", ["docs", "docs_win70_lens"])
@pytest.mark.parametrize("family", kr.ATTN_FAMILIES)
@pytest.mark.parametrize("h,hkv", [(4, 4), (4, 2)])
@pytest.mark.parametrize("d", [64, 128])
def test_band_packed_rope_against_fp64(d, h, hkv, family, band):
    """rope_qkv_flash_attention on the packed buffer.  The Function
    rotates q and k in place, so the buffer afterwards holds the bf16
    operands the attention kernels read: the reference takes those.  dv
    is compared as it is.  dq and dk come back rotated into the input
    frame and rounded once more: with R the (orthogonal, element i with
    i +- D/2, |cos|, |sin| <= 1) rotation back, the limit is
    F (E + roll(E)) on R ref plus one bf16 rounding of the result."""
    from easyparallellibrary_amd.ops.rope import (
        _rope_torch, rope_qkv_flash_attention, rope_tables)
    seq, ids, window, lens = band_of(band)
    q, k, v, dout = inputs(family, seq, d, h, hkv, valid_of(band), lens)
    flat = torch.cat([t.transpose(1, 2) for t in (q, k, v)], 2).reshape(
        B, seq, (h + 2 * hkv) * d).to(BF16).cuda().requires_grad_()
    buf = flat * 1
    sl = None if lens is None else torch.tensor(lens, dtype=torch.int32,
                                                device="cuda")
    out = rope_qkv_flash_attention(
        buf, num_heads=h, num_kv_heads=hkv, seqlens=sl, window=window,
        segment_ids=ids.cuda())
    out.backward(dout.to(BF16).cuda())
    rq, rk, rv = (t.to(F64) for t in buf.detach().cpu().view(
        B, seq, h + 2 * hkv, d).transpose(1, 2).split([h, hkv, hkv], 1))
    ref, bounds = reference(rq, rk, rv, dout, valid_of(band))
    cos, sin = (t[:seq].to(F64) for t in rope_tables("cpu", d))
    for name in ("dq", "dk"):
        ref[name] = _rope_torch(ref[name], cos, -sin)
        e = bounds[name] + bounds[name].roll(d // 2, -1)
        bounds[name] = e + kr.U_BF16 / kr.ATTN_FACTOR[name] * (
            ref[name].abs() + kr.ATTN_FACTOR[name] * e)
    grad = flat.grad.cpu().view(B, seq, h + 2 * hkv, d).transpose(1, 2)
    gq, gk, gv = grad.split([h, hkv, hkv], 1)
    check(dict(out=out.detach().cpu(), dq=gq, dk=gk, dv=gv), ref, bounds,
          lens, "packed")


@pytest.mark.parametrize("lens", [None, [130, 77]])
@pytest.mark.parametrize("seq", [200, 384])
@pytest.mark.parametrize("h,hkv", [(4, 4), (4, 2)])
@pytest.mark.parametrize("d", [64, 128])
def test_trivial_band_gives_the_causal_bits(d, h, hkv, seq, lens):
    """one document and window >= S: the head phase is empty, the tile
    order and the bodies are the causal kernels', and a masked tile in
    which nothing is masked computes what a plain tile computes"""
    inp = inputs("randn", seq, d, h, hkv)
    want = run(*inp, None, None, lens, causal_call=True)
    ids = torch.full((B, seq), 5)
    got = run(*inp, *device_bounds(ids, seq + 3, seq), lens)
    for name in ("out", "dq", "dk", "dv"):
        assert torch.equal(got[name].view(torch.int16),
                           want[name].view(torch.int16)), name


@pytest.mark.parametrize("lo,hi", [(384 + 5, None), (None, 0), (-7, -7)])
@pytest.mark.parametrize("d", [64, 128])
def test_hostile_bounds_stay_inside_the_buffers(d, lo, hi):
    """bounds the kernels must clamp (kv_lo to [0, i], q_hi to [j + 1,
    len]): finite results, untouched guard rows; no value is asserted"""
    from easyparallellibrary_amd import _C
    seq, h = 384, 4
    lay = kr.attn_layout("plain", B, h, seq, d, "cuda")
    for name, t in zip(("q", "k", "v", "dout"),
                       inputs("randn", seq, d, h, h)):
        lay[name].copy_(t.to(BF16))
    lse, delta = (kr.attn_flat(B * h * seq, torch.float32, "cuda")
                  for _ in range(2))
    kv_lo = torch.full((B, seq), 0 if lo is None else lo, dtype=torch.int32,
                       device="cuda")
    q_hi = torch.full((B, seq), seq if hi is None else hi,
                      dtype=torch.int32, device="cuda")
    sl = torch.tensor([seq, 201], dtype=torch.int32, device="cuda")
    scale = d ** -0.5
    _C.attn_fwd_band(lay["q"], lay["k"], lay["v"], lay["out"], lse.view,
                     scale, kv_lo, sl)
    _C.attn_bwd_band(lay["q"], lay["k"], lay["v"], lay["out"], lay["dout"],
                     lse.view, delta.view, lay["dq"], lay["dk"], lay["dv"],
                     scale, kv_lo, q_hi, sl)
    torch.cuda.synchronize()
    for name in ("out", "dq", "dk", "dv"):
        assert bool(torch.isfinite(lay[name].float()).all()), name
    for name, buf in list(lay["buffers"].items()) + [("lse", lse),
                                                     ("delta", delta)]:
        assert buf.stray_writes() == 0, name


@pytest.mark.parametrize("d,hkv", [(64, 4), (128, 2)])
def test_band_is_deterministic(d, hkv):
    seq, ids, window, lens = band_of("docs_win70_lens")
    inp = inputs("peaked", seq, d, 4, hkv, valid_of("docs_win70_lens"),
                 lens)
    bounds = device_bounds(ids, window, seq)
    a, b = run(*inp, *bounds, lens), run(*inp, *bounds, lens)
    for name in a:
        bits = torch.int16 if a[name].dtype == BF16 else torch.int32
        assert torch.equal(a[name].view(bits), b[name].view(bits)), name


class _PackedLlama(torch.nn.Module):
    """a llama whose rows always hold the same two documents"""

    def __init__(self, core, seg):
        super().__init__()
        self.core = core
        self.register_buffer("seg", seg)

    def forward(self, ids):
        return self.core(ids, self.seg)


def _train(graphed, steps=6):
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.models import llama
    from easyparallellibrary_amd.ops.distributed_losses import (
        ParallelCrossEntropy)
    epl.init(epl.Config({"kernel.hip_graph": graphed}))
    torch.manual_seed(5)
    core = llama.build_llama("llama-tiny-swa", vocab_size=128, max_pos=128)
    model = _PackedLlama(core, doc_ids(128, (50,))[None].repeat(4, 1).cuda())
    engine = epl.Engine(model, loss_fn=ParallelCrossEntropy(),
                        optimizer="adamw", lr=1e-3, dtype=torch.bfloat16)
    ids, tgt = (t.to(engine.device) for t in llama.synthetic_lm_batch(
        4, 128, 128, seed=11))
    losses = [float(engine.train_step(ids, tgt)) for _ in range(steps)]
    torch.cuda.synchronize()
    return engine, losses


def test_band_llama_hipgraph_step_matches_eager():
    """several replays of a captured llama-tiny-swa step with segment_ids
    against the eager steps, as test_llama_hipgraph_step_matches_eager"""
    engine_g, losses_g = _train(True)
    assert engine_g._hipgraph.graph is not None
    engine_e, losses_e = _train(False)
    assert engine_e._hipgraph is False
    for lg, le in zip(losses_g, losses_e):
        assert abs(lg - le) <= 0.05 * abs(le) + 1e-2, (losses_g, losses_e)
    assert losses_g[-1] < losses_g[0]
