"""Flash attention forward on inputs that move its running row maximum
(attn_fwd_softmax_cases.py), against the fp64 reference of kernel_refs.py.

The forward keeps the running maximum of a row on raw scores, exponentiates
with exp2 and a folded scale, and rescales its accumulators only when a row
of the wave has outgrown the maximum by more than 2^RESCALE_THR
(docs/kernels.md).  test_attention_fp64_gpu.py stops at seq 257 and its
inputs do not steer the maximum; the families here do: staircases whose
step sits below, just below, just above and far above the threshold, a
spike at the last key, a maximum at the first key, equal scores, and all
of these dealt to the rows of one wave.

Direct _C.attn_fwd calls, B = 2, H = 3.  Every case asserts
|out - ref| <= 2 E_out, lse within E_lse (kernel_refs.attn_bounds;
test_attention_fwd_softmax_refs_cpu.py shows the rounding model inside
1 x E on the same inputs), every result finite, and every guard element
around out, lse and the mask words untouched.  One case runs
_C.attn_bwd on the forward's out and lse and holds dq, dk, dv to 2 x E.
Each case prints its worst err / E (``ATTN-SOFTMAX`` lines).
"""

import pytest
import torch

from tests import attn_fwd_softmax_cases as sc
from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

F64 = torch.float64
B, H = sc.B, sc.H
SEED = (77 << 32) + 12345
FACTOR = dict(out=2.0, lse=1.0, dq=2.0, dk=2.0, dv=2.0)


class Run:
    """one forward (and optionally backward) through the kernels"""

    def __init__(self, inp, d, causal, thresh=0, lens=None, backward=False):
        from easyparallellibrary_amd import _C
        seq = inp[0].shape[2]
        lay = kr.attn_layout("plain", B, H, seq, d, "cuda")
        for key, t in zip(("q", "k", "v", "dout"), inp):
            lay[key].copy_(t.to(torch.bfloat16))
        flat = {"lse": kr.attn_flat(B * H * seq, torch.float32, "cuda"),
                "delta": kr.attn_flat(B * H * seq, torch.float32, "cuda")}
        mask = None
        if thresh:
            flat["mask"] = kr.attn_flat(B * H * seq * ((seq + 31) // 32),
                                        torch.int32, "cuda")
            mask = flat["mask"].view
            mask.fill_(0)
        tail = ()
        if lens is not None:
            tail = (torch.tensor(lens, dtype=torch.int32, device="cuda"),)
        scale = d ** -0.5
        inv_keep = kr.attn_inv_keep(thresh)
        _C.attn_fwd(lay["q"], lay["k"], lay["v"], lay["out"],
                    flat["lse"].view, scale, causal, mask, SEED, thresh,
                    inv_keep, *tail)
        names = ["out"]
        if backward:
            _C.attn_bwd(lay["q"], lay["k"], lay["v"], lay["out"],
                        lay["dout"], flat["lse"].view, flat["delta"].view,
                        lay["dq"], lay["dk"], lay["dv"], scale, causal, True,
                        mask, inv_keep, None, *tail)
            names += ["dq", "dk", "dv"]
        torch.cuda.synchronize()
        self.got = {name: lay[name].cpu().to(F64) for name in names}
        self.got["lse"] = flat["lse"].view.cpu().reshape(B, H, seq).to(F64)
        self.words = None if mask is None else mask.cpu()
        bufs = dict(lay["buffers"], **flat)
        self.stray = {key: buf.stray_writes() for key, buf in bufs.items()}
        self.seq = seq


def check(label, run, exp):
    ratios = {name: kr.attn_ratio((got - exp[name][0]).abs(), exp[name][1])
              for name, got in run.got.items()}
    print("ATTN-SOFTMAX {} {}".format(label, " ".join(
        "{}={:.3f}".format(n, r) for n, r in sorted(ratios.items()))))
    bad = ["{} err/E {:.3f} > {}".format(n, r, FACTOR[n])
           for n, r in ratios.items() if not r <= FACTOR[n]]
    bad += ["{} not finite".format(n) for n, t in run.got.items()
            if not bool(torch.isfinite(t).all())]
    bad += ["{} stray writes in {}".format(n, key)
            for key, n in run.stray.items() if n]
    assert not bad, (label, bad)


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("seq", sc.SEQS)
@pytest.mark.parametrize("d", sc.DIMS)
def test_forward(d, seq, causal, family):
    inp, exp = sc.case(family, seq, d, causal)
    check("d{} s{} causal{} {}".format(d, seq, int(causal), family),
          Run(inp, d, causal), exp)


def test_forward_dropout():
    """threshold 128 at seq 129: the reference is fed the published mask;
    l, and with it lse, accumulate undropped values"""
    d, seq, causal = 64, sc.DROP_SEQ, False
    inp = sc.inputs("mixed", seq, d)
    run = Run(inp, d, causal, sc.DROP_THRESH)
    keep = kr.unpack_keep(run.words, B * H, seq).reshape(B, H, seq, seq)
    rate = float(keep.mean())
    assert 0.4 < rate < 0.6, rate
    check("d{} s{} causal0 mixed thresh{}".format(d, seq, sc.DROP_THRESH),
          run, sc.expected(inp, d, causal, keep, sc.DROP_THRESH))


@pytest.mark.parametrize("causal", [False, True])
def test_forward_lengths(causal):
    """lengths 70 and 300 of 320: rows past a sample's length are exact
    zeros (they enter at a bound of zero), its keys past it are unused"""
    d, seq = 64, sc.LENS_SEQ
    inp, exp = sc.case("mixed", seq, d, causal, sc.LENS)
    check("d{} s{} lens{} causal{} mixed".format(
        d, seq, "/".join(map(str, sc.LENS)), int(causal)),
        Run(inp, d, causal, lens=sc.LENS), exp)


def test_backward_consumes_forward_lse():
    """staircase just above the threshold, five tiles: dq, dk, dv come
    from the forward's out and lse"""
    d, seq, causal = 64, 320, False
    family = "staircase{:g}".format(sc.RESCALE_THR + 0.5)
    inp, exp = sc.case(family, seq, d, causal)
    check("d{} s{} causal0 {} backward".format(d, seq, family),
          Run(inp, d, causal, backward=True), exp)
