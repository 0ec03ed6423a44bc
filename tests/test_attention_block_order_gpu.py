"""The XCD-local block order of the non-causal attention grids
(csrc/kernels/attn_block_order.h).

* The map itself, read back from a probe kernel launched on the real grid
  shape dim3(n, BH): it is a permutation of all (bh, blk), and the blocks
  with equal L % 8 walk, in the order of L / 8, one batch-head's blocks
  before the next batch-head's.
* Forward and backward against the fp64 reference at batch*heads of 7, 8,
  9, 16 and 17 — the other attention suites mostly run six batch-heads,
  where the map is the identity — with the reference, the bounds and the
  factors of test_attention_fp64_gpu.py / test_attention_varlen_gpu.py
  (kernel_refs.attn_bounds at kernel_refs.ATTN_FACTOR), in every layout of
  kernel_refs.ATTN_LAYOUTS.  A wrong (bh, blk) computes another tile or
  leaves one unwritten; the NaN sentinels of the guarded buffers show
  either.
"""

import pytest
import torch

from tests import attn_gpu_runs as ar
from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1), (1, 7), (4, 8), (4, 9), (3, 8), (2, 17), (5, 24), (4, 16)]
# batch*heads -> (B, H)
SHAPES = {7: (1, 7), 8: (2, 4), 9: (3, 3), 16: (2, 8), 17: (1, 17)}
# with lengths: enough samples for an empty, a one-token and a full one
LEN_SHAPES = {7: (7, 1), 8: (4, 2), 9: (3, 3), 16: (4, 4), 17: (17, 1)}
SEQS = (128, 129, 200)


@pytest.mark.parametrize("n,bh", GRIDS)
def test_block_order_map(n, bh):
    from easyparallellibrary_amd import _C
    out = torch.full((n * bh, 2), -1, dtype=torch.int32, device="cuda")
    _C.attn_block_order_probe(out, n, bh)
    torch.cuda.synchronize()
    got = [tuple(p) for p in out.cpu().tolist()]
    # a permutation of all (bh, blk)
    assert sorted(got) == [(h, k) for h in range(bh) for k in range(n)]
    # below n * BH8: the blocks that share L % 8 take, in the order of
    # L / 8, the n blocks of a batch-head, then those of the next one
    bh8 = bh & ~7
    for g in range(8):
        walk = [got[L] for L in range(g, n * bh8, 8)]
        assert walk == [(8 * t + g, k) for t in range(bh8 // 8)
                        for k in range(n)], (g, walk)
    # the rest keeps its place
    for L in range(n * bh8, n * bh):
        assert got[L] == (L // n, L % n)


def _family(index):
    return kr.ATTN_FAMILIES[index % len(kr.ATTN_FAMILIES)]


DENSE = [(d, seq, nbh) for d in kr.ATTN_DIMS for seq in SEQS
         for nbh in sorted(SHAPES)]


@pytest.mark.parametrize(
    "index", range(len(DENSE)),
    ids=["d{}-s{}-bh{}".format(*c) for c in DENSE])
def test_fp64_dense(index):
    d, seq, nbh = DENSE[index]
    b, h = SHAPES[nbh]
    family = _family(index)
    inp = kr.attn_inputs(family, seq, d, False, b=b, h=h)
    exp = ar.expected(inp, d, False)
    runs = []
    for layout in kr.ATTN_LAYOUTS:
        run = ar.Run(inp, d, False, layout)
        ar.check("block-order", "d{} s{} b{} h{} {} {}".format(
            d, seq, b, h, family, layout), run, exp)
        runs.append(run)
    # the layout moves no bit
    for run in runs[1:]:
        assert not ar.differing(runs[0], run)
    # the combined dK+dV kernel takes the same order and gives the same bits
    if d == 64:
        assert not ar.differing(
            runs[0], ar.Run(inp, d, False, "qkv", split=False))


@pytest.mark.parametrize("nbh", sorted(LEN_SHAPES))
def test_fp64_lengths(nbh):
    b, h = LEN_SHAPES[nbh]
    d = 64 if nbh % 2 else 128
    seq = 200
    lens = tuple((0, 1, seq, 129, 65, 128, 33)[i % 7] for i in range(b))
    assert {0, 1, seq} <= set(lens)
    family = _family(nbh)
    inp = kr.attn_inputs(family, seq, d, False, b=b, h=h)
    exp = ar.expected(inp, d, False, lens)
    for layout in kr.ATTN_LAYOUTS:
        ar.check("block-order-lengths", "d{} s{} b{} h{} {} {}".format(
            d, seq, b, h, family, layout),
            ar.Run(inp, d, False, layout, lens), exp)


def test_causal_grid_untouched():
    """batch*heads = 16, causal: the grid and its order are the old ones"""
    b, h = SHAPES[16]
    for d in kr.ATTN_DIMS:
        inp = kr.attn_inputs("randn", 200, d, True, b=b, h=h)
        exp = ar.expected(inp, d, True)
        for layout in kr.ATTN_LAYOUTS:
            ar.check("block-order-causal", "d{} s200 b{} h{} {}".format(
                d, b, h, layout), ar.Run(inp, d, True, layout), exp)
