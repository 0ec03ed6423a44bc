"""Inputs that move the running max of the attention forward's online
softmax, shared by test_attention_fwd_softmax_refs_cpu.py and
test_attention_fwd_softmax_gpu.py (not a test file).

The forward walks the keys in 32-key sub-tiles and keeps a running row
maximum m.  It rescales its accumulators only when some row of the wave
has outgrown m by more than T = RESCALE_THR powers of two (kRescaleThr in
csrc/kernels/attention.hip); otherwise it keeps the stale m.  The families
below steer, per query row, how the row maximum moves from one sub-tile to
the next.  "Steps" are in the exponent domain: differences of
score * log2(e).

Construction.  Coordinate f of q selects profile f for that row: a row of
profile f holds QSEL (about ln 2, bf16-exact) at coordinate f and zeros at
the other profile coordinates, and k[j][f] = g_f(j) / scale, so the row's
score is QSEL * g_f(j) plus O(0.1) noise from the coordinates above the
profiles.  Everything is rounded to bf16 before use, so kernel and
reference see the same numbers.

    staircase step : g(j) = (j // 32) * step; steps STAIR_STEPS
    late_spike     : g = 0 and g(len - 1) = 80
    descending     : g(j) = -j / 4, the maximum is key 0
    constant       : the q row is all zero, every score is equal
    mixed          : the profiles above dealt to consecutive rows, so the
                     rows of one wave disagree about the rescale
"""

import functools
import math

import torch

from tests import kernel_refs as kr

F64 = torch.float64
B, H = kr.ATTN_B, kr.ATTN_H
RESCALE_THR = 8.0
STAIR_STEPS = (0.25, RESCALE_THR - 0.5, RESCALE_THR + 0.5, 4 * RESCALE_THR)
PROFILES = tuple("staircase{:g}".format(s) for s in STAIR_STEPS) + (
    "late_spike", "descending", "constant")
FAMILIES = PROFILES + ("mixed",)
QSEL = 0.69140625          # bf16 nearest ln 2: a step of g is a power of two
NOISE = 0.25
DIMS = (64, 128)
SEQS = (64, 65, 129, 320)  # 320: five tiles, both staging buffers reused
DROP_SEQ, DROP_THRESH = 129, 128
LENS_SEQ, LENS = 320, (70, 300)


def _profile(name, seq, lens):
    """g_f(j) for every sample: fp64 [B, seq]"""
    j = torch.arange(seq, dtype=F64)
    if name.startswith("staircase"):
        g = torch.div(j, 32, rounding_mode="floor") * float(name[9:])
        return g.expand(B, seq).clone()
    if name == "late_spike":
        g = torch.zeros(B, seq, dtype=F64)
        for b, n in enumerate(lens):
            g[b, n - 1] = 80.0
        return g
    if name == "descending":
        return (-j / 4).expand(B, seq).clone()
    assert name == "constant"
    return torch.zeros(B, seq, dtype=F64)


def inputs(family, seq, d, lens=None, seed=0):
    """q, k, v, dout: fp64 [B,H,seq,d] of bf16-representable values.  lens:
    per-sample valid lengths (the late spike sits at len - 1), default
    seq."""
    assert family in FAMILIES
    lens = (seq,) * B if lens is None else tuple(lens)
    gen = torch.Generator().manual_seed(
        9000 + seed + 31 * FAMILIES.index(family) + 7 * seq + d)
    scale = 1.0 / math.sqrt(d)
    q, k, v, dout = (torch.randn(B, H, seq, d, generator=gen, dtype=F64)
                     for _ in range(4))
    n = len(PROFILES)
    q[..., :n] = 0.0
    q[..., n:] *= NOISE
    k[..., n:] *= NOISE
    rows = torch.arange(seq)
    for f, name in enumerate(PROFILES):
        k[..., f] = (_profile(name, seq, lens) / scale)[:, None, :]
        if family == "mixed":
            mine = rows % n == f
        else:
            mine = torch.full((seq,), family == name)
        if name == "constant":
            q[:, :, mine] = 0.0
        else:
            q[:, :, mine, f] = QSEL
    return tuple(kr.bf16_round(t) for t in (q, k, v, dout))


def expected(inp, d, causal, keep=None, thresh=0, lens=None):
    """reference and bounds: {name: (want, bound)} for out, lse, dq, dk,
    dv.  With lens, sample b is the dense problem on its first lens[b]
    rows and keys, and everything past them is zero at a bound of zero."""
    scale = d ** -0.5
    inv_keep = kr.attn_inv_keep(thresh)
    names = ("out", "lse", "dq", "dk", "dv")
    if lens is None:
        ref = kr.attn_ref(*inp, causal, scale, keep, inv_keep)
        bounds = kr.attn_bounds(ref, *inp, scale)
        return {name: (ref[name], bounds[name]) for name in names}
    res = {name: (torch.zeros(inp[0].shape[:3] if name == "lse"
                              else inp[0].shape, dtype=F64),
                  torch.zeros(inp[0].shape[:3] if name == "lse"
                              else inp[0].shape, dtype=F64))
           for name in names}
    for b, n in enumerate(lens):
        part = tuple(t[b:b + 1, :, :n] for t in inp)
        kp = None if keep is None else keep[b:b + 1, :, :n, :n]
        ref = kr.attn_ref(*part, causal, scale, kp, inv_keep)
        bounds = kr.attn_bounds(ref, *part, scale)
        for name in names:
            res[name][0][b, :, :n] = ref[name][0]
            res[name][1][b, :, :n] = bounds[name][0]
    return res


@functools.lru_cache(maxsize=None)
def case(family, seq, d, causal, lens=None):
    """(inputs, expected) of a case without dropout, computed once"""
    inp = inputs(family, seq, d, lens)
    return inp, expected(inp, d, causal, lens=lens)


def max_steps(inp, d, causal):
    """largest rise of the running row maximum between consecutive 32-key
    sub-tiles, in the exponent domain, over all rows: what the family
    actually asks of the rescale decision"""
    q, k = inp[0], inp[1]
    seq = q.shape[2]
    s = torch.matmul(q, k.transpose(-1, -2)) * d ** -0.5 * math.log2(math.e)
    s = s.masked_fill(~kr.attn_valid(seq, seq, causal), float("-inf"))
    pad = (-seq) % 32
    if pad:
        s = torch.nn.functional.pad(s, (0, pad), value=float("-inf"))
    tiles = s.reshape(B, H, seq, -1, 32).max(dim=-1).values
    run = torch.cummax(tiles, dim=-1).values
    rise = run[..., 1:] - run[..., :-1]
    rise = rise[torch.isfinite(rise)]
    return float(rise.max()) if rise.numel() else 0.0
