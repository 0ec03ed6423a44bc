"""The padded-batch attention reference of varlen_refs.py, checked on the
CPU: it is what torch autograd computes under the boolean mask, the
kernels' rounding model stays inside the unchanged bounds on every case of
the GPU matrix (test_attention_varlen_gpu.py), and the criterion rejects
seven wrong ways of handling the lengths."""

import pytest
import torch

from tests import kernel_refs as kr
from tests import varlen_refs as vr

F64 = torch.float64
B, H = vr.B, vr.H


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("family", kr.ATTN_FAMILIES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("thresh,with_dlse", [(0, False), (128, True)])
def test_varlen_ref_matches_autograd(family, causal, thresh, with_dlse):
    for seq, lens, d in ((72, (72, 37), 64), (72, (1, 64), 128),
                         (200, (65, 127), 64)):
        inp = kr.attn_inputs(family, seq, d, causal)
        q, k, v, dout = inp
        scale = d ** -0.5
        keep = vr.cpu_keep(seq, thresh)
        inv_keep = kr.attn_inv_keep(thresh)
        dlse = kr.attn_dlse(seq) if with_dlse else None
        lb = vr.lens_b1(lens)
        ref = vr.model(inp, lb, causal, scale, keep, inv_keep, dlse)
        for t in ref.values():
            assert t is None or bool(torch.isfinite(t.to(F64)).all())
        qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
        mask = vr.valid_mask(seq, lb, causal)
        s = torch.matmul(qa, ka.transpose(-1, -2)) * scale
        s = s.masked_fill(~mask, float("-inf"))
        p = torch.softmax(s, dim=-1)
        if keep is not None:
            p = p * keep * inv_keep
        rows = vr.row_mask(seq, lb).to(F64)
        out = torch.matmul(p, va) * rows[..., None]
        lse = torch.logsumexp(s, dim=-1) * rows
        dl = dlse if dlse is not None else torch.zeros_like(lse)
        # the padded rows of out and lse are constants (zero), so whatever
        # cotangent arrives there reaches nothing
        gq, gk, gv = torch.autograd.grad([out, lse], [qa, ka, va],
                                         [dout, dl])
        for name, want in (("out", out.detach()), ("lse", lse.detach()),
                           ("dq", gq), ("dk", gk), ("dv", gv)):
            assert _rel(ref[name], want) < 1e-12, (name, seq, lens, d)
        # exact zeros on the padded rows once dout is zeroed there
        for b, n in enumerate(lens):
            for name in ("dq", "dk", "dv", "out", "lse"):
                assert not bool(ref[name][b, :, n:].any()), (name, b)


def _emulation_ratios(inp, lens, d, causal, thresh=0, dlse=None):
    seq = inp[0].shape[2]
    keep = vr.cpu_keep(seq, thresh)
    exp = vr.Expected(inp, lens, d, causal, keep, thresh, dlse)
    emu = vr.model(inp, vr.lens_b1(lens).clamp(min=1), causal, d ** -0.5,
                   keep, kr.attn_inv_keep(thresh), dlse, emulate=True)
    # the kernels write an empty sample as zeros; the model ran it as
    # length 1
    for b, n in enumerate(lens):
        if n == 0:
            for name in kr.ATTN_OUTPUTS:
                emu[name][b] = 0.0
    return exp.ratios(emu)


def _assert_inside(label, ratios, worst):
    for name, r in ratios.items():
        worst[name] = max(worst.get(name, 0.0), r)
        assert r <= 1.0, (label, name, r)


def test_varlen_emulation_inside_bounds_main():
    worst = {}
    for index, (d, seq, lens, causal) in enumerate(vr.MAIN):
        family = vr.main_family(index)
        inp = kr.attn_inputs(family, seq, d, causal)
        _assert_inside((d, seq, lens, causal, family),
                       _emulation_ratios(inp, lens, d, causal), worst)
    print(worst)


def test_varlen_emulation_inside_bounds_dropout_dlse_combined():
    worst = {}
    for d in kr.ATTN_DIMS:
        for seq, lens in vr.DROP_CASES:
            for causal in (False, True):
                inp = kr.attn_inputs("randn", seq, d, causal)
                _assert_inside(("drop", d, seq, lens, causal),
                               _emulation_ratios(inp, lens, d, causal,
                                                 vr.DROP_THRESH), worst)
    for d, seq, lens, causal in vr.DLSE_CASES:
        for family in kr.ATTN_FAMILIES:
            inp = kr.attn_inputs(family, seq, d, causal)
            _assert_inside(("dlse", d, seq, lens, causal, family),
                           _emulation_ratios(inp, lens, d, causal,
                                             dlse=kr.attn_dlse(seq)), worst)
    for seq, lens in vr.COMBINED_CASES:
        for family in kr.ATTN_FAMILIES:
            inp = kr.attn_inputs(family, seq, 64, False)
            _assert_inside(("combined", seq, lens, family),
                           _emulation_ratios(inp, lens, 64, False), worst)
    print(worst)


def test_varlen_emulation_inside_bounds_env_cases():
    worst = {}
    for d, seq, lens, causal, thresh, family in vr.env_cases(0):
        inp = kr.attn_inputs(family, seq, d, causal)
        _assert_inside((d, seq, lens, causal, thresh, family),
                       _emulation_ratios(inp, lens, d, causal, thresh),
                       worst)
    print(worst)


# ---------------------------------------------------------------------------
# wrong kernels: each must exceed ATTN_FACTOR x E at least tenfold somewhere
# ---------------------------------------------------------------------------
MUTATIONS = ("padded_key_counted", "last_valid_key_dropped",
             "lengths_exchanged", "length_by_bh_mod_b",
             "padded_queries_in_dk_dv", "padded_out_rows_left",
             "causal_dropped_with_lengths")


def _mutants(inp, lens, causal, scale):
    """name -> outputs of a wrong kernel; the padding of the inputs is
    finite (what attn_inputs generated there)"""
    seq = inp[0].shape[2]
    lb = vr.lens_b1(lens)
    m = {
        "padded_key_counted": vr.model(
            inp, lb, causal, scale, key_lbh=(lb + 1).clamp(max=seq)),
        "last_valid_key_dropped": vr.model(
            inp, lb, causal, scale, key_lbh=(lb - 1).clamp(min=1)),
        "lengths_exchanged": vr.model(inp, lb.flip(0), causal, scale),
        # the length of batch-head bh read at bh % B, not bh / heads
        "length_by_bh_mod_b": vr.model(
            inp, torch.tensor([[lens[(b * H + h) % B] for h in range(H)]
                               for b in range(B)]), causal, scale),
        "padded_queries_in_dk_dv": vr.model(inp, lb, causal, scale,
                                            zero_dout=False),
        "padded_out_rows_left": vr.model(inp, lb, causal, scale,
                                         zero_rows=False),
    }
    if causal:
        m["causal_dropped_with_lengths"] = vr.model(inp, lb, causal, scale,
                                                    keep_causal=False)
    return m


@pytest.fixture(scope="module")
def mutation_ratios():
    """{mutation: {case: worst err / (factor * E)}} over a slice of the GPU
    matrix (no empty sample: every mutant needs lengths >= 1)"""
    res = {name: {} for name in MUTATIONS}
    cases = ((64, 72, (72, 37)), (64, 200, (65, 127)), (128, 257, (32, 129)),
             (128, 200, (128, 63)))
    for i, (d, seq, lens) in enumerate(cases):
        for causal in (False, True):
            family = kr.ATTN_FAMILIES[i % len(kr.ATTN_FAMILIES)]
            inp = kr.attn_inputs(family, seq, d, causal)
            exp = vr.Expected(inp, lens, d, causal)
            # the criterion accepts the right kernel ...
            good = exp.ratios(vr.model(inp, vr.lens_b1(lens), causal,
                                       d ** -0.5))
            assert max(good.values()) == 0.0, good
            # ... and is scaled by the allowed factor for the wrong ones
            for name, outs in _mutants(inp, lens, causal,
                                       d ** -0.5).items():
                ratios = exp.ratios(outs)
                res[name][(family, d, seq, lens, causal)] = max(
                    ratios[o] / kr.ATTN_FACTOR[o]
                    for o in ("out", "lse", "dq", "dk", "dv"))
    return res


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_varlen_criterion_rejects_mutation(mutation_ratios, mutation):
    ratios = mutation_ratios[mutation]
    assert ratios, mutation
    best = max(ratios, key=ratios.get)
    print(mutation, "worst err / allowed:", ratios[best], "at", best,
          "; weakest case:", min(ratios.values()))
    assert ratios[best] >= 10.0, (mutation, best, ratios[best])
