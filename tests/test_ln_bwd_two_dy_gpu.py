"""LayerNorm backward with two upstream gradients (the DY2 form of
layer_norm_bwd_bf16_kernel, csrc/kernels/kernels.hip) against the fp64
reference of kernel_refs.py.

The kernel forms dy + dy2 in fp32 right after the loads and never rounds
the sum to bf16.  dy and dy2 come from two seeds of the dy families of
kernel_refs.py and are fixed up on the CPU so that every fp32 sum is
exact (asserted in fp64 before the launch: two 8-bit mantissas fit the 24
bits of fp32 when their exponents are at most 15 apart; the few pairs
further apart take dy2 = 0).  The reference and the derived bound are
then ln_bwd_ref / ln_bwd_bounds at that exact sum, applied as
test_layer_norm_fp64_gpu.py applies them (kr.LN_FACTOR_BF16: 2 E on the
bf16 dx, E on dgamma, dbeta and colsum).

Shapes: cols 256 / 1000 / 1024 / 2048 (CHUNKS 1 / 2 / 2 / 4, one width
that is no multiple of 512) x rows 1 / 3 / 5 / 4100 (4100 > 4 x 1024: some
waves take a second row), each with and without dadd and the column sum.
Also: dy2 = 0 gives the bits of the single-dy call, swapping dy and dy2
gives equal bits, and no guard element around an output is written.
"""

import pytest
import torch

from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

F64 = torch.float64
COLS = (256, 1000, 1024, 2048)
ROWS = (1, 3, 5, 4100)


def two_dy(rows, cols, name):
    """dy, dy2 (bf16-representable fp64) whose sum is exact in fp32"""
    g1 = torch.Generator().manual_seed(11 + rows + 3 * cols)
    g2 = torch.Generator().manual_seed(977 + rows + 3 * cols)
    dy = kr.dy_family(name, rows, cols, g1)
    dy2 = kr.dy_family(name, rows, cols, g2)
    s = dy + dy2
    inexact = kr.f32_round(s) != s
    # the families sit within a 2^15 ratio almost everywhere
    assert float(inexact.double().mean()) < 1e-3
    dy2 = torch.where(inexact, torch.zeros_like(dy2), dy2)
    s = dy + dy2
    assert torch.equal(kr.f32_round(s), s)
    assert torch.equal(kr.bf16_round(dy2), dy2)
    return dy, dy2, s


def launch(c, rows, cols, x, gamma, mean, rstd, dy, dy2, dadd, want_cs,
           out_dtype=torch.float32):
    """layer_norm_bwd_typed into guarded, NaN-filled outputs; returns the
    device results (raw, for bit comparisons) and the stray-write list"""
    bf = torch.bfloat16

    def dev(t):
        return None if t is None else t.to(bf).cuda().contiguous()

    bufs = {"dx": kr.guarded_rows(rows, cols, bf, "cuda"),
            "dgamma": kr.attn_flat(cols, out_dtype, "cuda"),
            "dbeta": kr.attn_flat(cols, out_dtype, "cuda")}
    if want_cs:
        bufs["colsum"] = kr.attn_flat(cols, out_dtype, "cuda")
    c.layer_norm_bwd_typed(
        bufs["dx"].view, bufs["dgamma"].view, bufs["dbeta"].view, dev(dy),
        dev(x), dev(gamma), mean.float().cuda(), rstd.float().cuda(),
        dev(dadd), bufs["colsum"].view if want_cs else None, dev(dy2))
    torch.cuda.synchronize()
    stray = ["%d stray writes around %s" % (b.stray_writes(), k)
             for k, b in bufs.items() if b.stray_writes()]
    return {k: b.view.clone() for k, b in bufs.items()}, stray


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_two_dy_backward(rows, cols):
    from easyparallellibrary_amd import _C
    name = "cancel" if rows % 2 else "coherent"
    if rows == 5:
        name = "coherent"
    inp = kr.ln_inputs(rows, cols, False)
    x, gamma = inp["x"], inp["gamma"]
    fwd = kr.ln_ref(x, None, gamma, inp["beta"])
    # the kernel is handed fp32 statistics: the reference takes the same
    mean, rstd = kr.f32_round(fwd["mean"]), kr.f32_round(fwd["rstd"])
    dy, dy2, dsum = two_dy(rows, cols, name)
    bad, worst, refs = [], {}, {}
    for use_dadd, use_cs in kr.LN_FLAGS:
        dadd = inp["dadd"] if use_dadd else None
        if use_dadd not in refs:      # one reference per dadd setting
            r = kr.ln_bwd_ref(dsum, x, gamma, mean, rstd, dadd)
            refs[use_dadd] = (r, kr.ln_bwd_bounds(
                r, dsum, x, gamma, mean, rstd, dadd, True))
        ref, e = refs[use_dadd]
        got, stray = launch(_C, rows, cols, x, gamma, mean, rstd, dy, dy2,
                            dadd, use_cs)
        bad += stray
        label = "dadd%d cs%d" % (use_dadd, use_cs)
        for key in ("dx", "dgamma", "dbeta") + (("colsum",) if use_cs
                                                else ()):
            r = kr.ratio_of(got[key].cpu().to(F64), ref[key], e[key])
            worst[key] = max(worst.get(key, 0.0), r)
            if not r <= kr.LN_FACTOR_BF16[key]:
                bad.append("%s %s err/E %.3g" % (label, key, r))
        # dy2 = 0: the single-dy kernel's bits; swapped: the same bits
        zero, _ = launch(_C, rows, cols, x, gamma, mean, rstd, dy,
                         torch.zeros_like(dy), dadd, use_cs)
        one, _ = launch(_C, rows, cols, x, gamma, mean, rstd, dy, None,
                        dadd, use_cs)
        swap, _ = launch(_C, rows, cols, x, gamma, mean, rstd, dy2, dy,
                         dadd, use_cs)
        for key in got:
            if not torch.equal(zero[key], one[key]):
                bad.append("%s %s: dy2 = 0 differs from single dy"
                           % (label, key))
            if not torch.equal(swap[key], got[key]):
                bad.append("%s %s: swapped dy, dy2 differ" % (label, key))
    print("LN2DY-RATIO cols %d rows %d %s %s" % (cols, rows, name, " ".join(
        "%s=%.3f" % kv for kv in sorted(worst.items()))))
    assert not bad, (bad[:8], len(bad))
