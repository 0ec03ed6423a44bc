"""The running-max input families of attn_fwd_softmax_cases.py, on the CPU.

test_attention_fwd_softmax_gpu.py holds the forward kernel to 2 x E on out
and 1 x E on lse (kernel_refs.attn_bounds) on these inputs.  This file
shows that the bound is sound there: kernel_refs.attn_emulate, which is
attn_ref with the kernels' bf16 roundings inserted, stays within 1 x E of
attn_ref on every element of out and within the lse bound, for every
family, shape and variant the GPU test runs, and on dq, dk, dv for the
input of its backward case.  (The gradients are not claimed for every
family: where a staircase spans more than the exponent range of bf16, as
staircase32 does at seq 320, P underflows and the relative bounds on dk
and dv no longer describe a flush to zero.)  It also checks that each
family moves the running maximum the way its name says, so a later edit of
the builders cannot quietly stop exercising the rescale decision.
"""

import pytest
import torch

from tests import attn_fwd_softmax_cases as sc
from tests import kernel_refs as kr

F64 = torch.float64
NAMES = ("out", "lse")
GRADS = ("dq", "dk", "dv")


def _ratios(inp, d, causal, exp, keep=None, thresh=0, names=NAMES):
    emu = kr.attn_emulate(*inp, causal, d ** -0.5, keep,
                          kr.attn_inv_keep(thresh))
    return {name: kr.attn_ratio((emu[name] - exp[name][0]).abs(),
                                exp[name][1]) for name in names}


def _check(label, ratios):
    print("ATTN-SOFTMAX-REF {} {}".format(label, " ".join(
        "{}={:.3f}".format(n, r) for n, r in ratios.items())))
    bad = {n: r for n, r in ratios.items() if not r <= 1.0}
    assert not bad, (label, bad)


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("seq", sc.SEQS)
@pytest.mark.parametrize("d", sc.DIMS)
def test_emulation_within_bounds(d, seq, causal, family):
    inp, exp = sc.case(family, seq, d, causal)
    for t in inp:
        assert torch.equal(t, kr.bf16_round(t))
    _check("d{} s{} causal{} {}".format(d, seq, int(causal), family),
           _ratios(inp, d, causal, exp))


def test_emulation_within_bounds_backward_case():
    d, seq, causal = 64, 320, False
    family = "staircase{:g}".format(sc.RESCALE_THR + 0.5)
    inp, exp = sc.case(family, seq, d, causal)
    _check("d{} s{} causal0 {} backward".format(d, seq, family),
           _ratios(inp, d, causal, exp, names=NAMES + GRADS))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", sc.DIMS)
def test_emulation_within_bounds_dropout(d, causal):
    seq = sc.DROP_SEQ
    inp = sc.inputs("mixed", seq, d)
    gen = torch.Generator().manual_seed(5)
    keep = (torch.rand(sc.B, sc.H, seq, seq, generator=gen) <
            1.0 - sc.DROP_THRESH / 256.0).to(F64)
    exp = sc.expected(inp, d, causal, keep, sc.DROP_THRESH)
    _check("d{} s{} causal{} mixed dropout".format(d, seq, int(causal)),
           _ratios(inp, d, causal, exp, keep, sc.DROP_THRESH))


@pytest.mark.parametrize("causal", [False, True])
def test_emulation_within_bounds_lengths(causal):
    """each sample of the padded case is the dense problem on its own
    length, and the expectation past it is zero at a bound of zero"""
    d, seq = 64, sc.LENS_SEQ
    inp, exp = sc.case("mixed", seq, d, causal, sc.LENS)
    for b, n in enumerate(sc.LENS):
        part = tuple(t[b:b + 1, :, :n] for t in inp)
        pexp = {name: (exp[name][0][b:b + 1, :, :n],
                       exp[name][1][b:b + 1, :, :n]) for name in NAMES}
        _check("d{} s{} len{} causal{} mixed".format(d, seq, n, int(causal)),
               _ratios(part, d, causal, pexp))
        for name in NAMES:
            assert not bool(exp[name][0][b, :, n:].any())
            assert not bool(exp[name][1][b, :, n:].any())


def test_families_move_the_running_max():
    """largest rise of the running maximum between sub-tiles, exponent
    domain, at seq 320 non-causal"""
    thr = sc.RESCALE_THR
    rise = {f: sc.max_steps(sc.case(f, 320, 64, False)[0], 64, False)
            for f in sc.FAMILIES}
    print("ATTN-SOFTMAX-RISE", rise)
    stairs = [rise["staircase{:g}".format(s)] for s in sc.STAIR_STEPS]
    # noise moves a step by a few tenths at the most
    assert 0.0 < stairs[0] < 1.0
    assert thr - 1.0 < stairs[1] < thr          # stays below the threshold
    assert thr < stairs[2] < thr + 1.0          # crosses it at every step
    assert 4 * thr - 1.0 < stairs[3] < 4 * thr + 1.0
    assert 75.0 < rise["late_spike"] < 85.0
    assert rise["descending"] == 0.0
    assert rise["constant"] == 0.0
    assert rise["mixed"] > 4 * thr - 1.0
    # mixed: the rows of one 32-row wave disagree
    inp = sc.case("mixed", 320, 64, False)[0]
    per_row = []
    for r in range(len(sc.PROFILES)):
        one = tuple(t[:, :, r:r + 1] if i in (0, 3) else t
                    for i, t in enumerate(inp))
        s = torch.matmul(one[0], one[1].transpose(-1, -2))[0, 0, 0]
        per_row.append(int(s.argmax()))
    assert len(set(per_row)) >= 3, per_row
