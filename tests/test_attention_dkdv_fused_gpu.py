"""The combined dK+dV kernel (attn_bwd_dkdv_kernel: d64, non-causal, no
dropout) against the split dV and dK kernels.

The combined tile runs the split tiles' MFMA chains, chunk order, sub-tile
order and ``exp2(...) * dp * scale`` expression in their order, so
``attn_bwd(..., split_dkdv=False)`` must give dq, dk, dv and delta (rows <
len) with the BITS of ``split_dkdv=True``.  B = 2, H = 4: eight batch-heads,
so the XCD-local block order is not the identity.

The seqs cover a single partial chunk (1, 31), exactly one chunk (64), both
LDS buffers and the prefetch guard at three or more chunks (129 ... 257), a
second kv block holding a single key (129, 257) and inactive waves (every
seq that is not a multiple of 128).

One fp64 bound check per seq (reference, bounds and factors of
test_attention_fp64_gpu.py) guards against both paths being wrong
together, and an ineligible call must take the split kernels whatever the
flag says.
"""

import pytest

from tests import attn_gpu_runs as ar
from tests import kernel_refs as kr
from tests import varlen_refs as vr

pytestmark = pytest.mark.gpu

B, H, D = 2, 4, 64
SEQS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257)
LEN_CASES = tuple(vr.COMBINED_CASES) + ((200, (0, 200)), (72, (0, 72)),
                                        (200, (1, 65)))


def _pair(inp, layout, lens=None, dlse=None, d=D, causal=False):
    split = ar.Run(inp, d, causal, layout, lens, dlse, split=True)
    fused = ar.Run(inp, d, causal, layout, lens, dlse, split=False)
    return split, fused


@pytest.mark.parametrize("seq", SEQS)
def test_fused_matches_split_dense(seq):
    family = kr.ATTN_FAMILIES[SEQS.index(seq) % len(kr.ATTN_FAMILIES)]
    inp = kr.attn_inputs(family, seq, D, False, b=B, h=H)
    exp = ar.expected(inp, D, False)
    for layout in kr.ATTN_LAYOUTS:
        split, fused = _pair(inp, layout)
        assert not ar.differing(split, fused), (
            layout, ar.differing(split, fused))
        assert not any(fused.stray.values()), fused.stray
    # both against fp64, once per seq
    ar.check("dkdv-fused", "d64 s{} {} {}".format(seq, family, layout),
             fused, exp)


@pytest.mark.parametrize("seq,lens", LEN_CASES)
def test_fused_matches_split_lengths(seq, lens):
    for i, family in enumerate(kr.ATTN_FAMILIES):
        inp = kr.attn_inputs(family, seq, D, False, b=B, h=H)
        layout = kr.ATTN_LAYOUTS[i]
        split, fused = _pair(inp, layout, lens)
        assert not ar.differing(split, fused), (
            family, ar.differing(split, fused))
        ar.check("dkdv-fused-lengths", "d64 s{} len{}-{} {} {}".format(
            seq, lens[0], lens[1], family, layout), fused,
            ar.expected(inp, D, False, lens))


@pytest.mark.parametrize("seq,lens", [(200, None), (200, (65, 127)),
                                      (129, None)])
def test_fused_matches_split_dlse(seq, lens):
    dlse = kr.attn_dlse(seq, b=B, h=H)
    assert float(dlse.abs().min()) > 0
    inp = kr.attn_inputs("randn", seq, D, False, b=B, h=H)
    exp = ar.expected(inp, D, False, lens, dlse)
    for layout in kr.ATTN_LAYOUTS:
        split, fused = _pair(inp, layout, lens, dlse)
        assert not ar.differing(split, fused), (
            layout, ar.differing(split, fused))
        ar.check("dkdv-fused-dlse", "d64 s{} {}".format(seq, layout), fused,
                 exp)


@pytest.mark.parametrize("d,causal", [(64, True), (128, False)])
def test_ineligible_call_runs_split(d, causal):
    seq = 200
    inp = kr.attn_inputs("randn", seq, d, causal, b=B, h=H)
    split, asked = _pair(inp, "qkv", d=d, causal=causal)
    assert not ar.differing(split, asked)
    ar.check("dkdv-ineligible", "d{} s{} causal{}".format(d, seq,
                                                          int(causal)),
             asked, ar.expected(inp, d, causal))
