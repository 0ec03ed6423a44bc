"""The XCD-local block order (csrc/kernels/attn_block_order.h) evaluated on
the host: a bijection for every grid, of the stated shape.  The GPU test
(test_attention_block_order_gpu.py) reads the same map back from the
blocks of real launches."""

import pytest


def _order(n, bh):
    from easyparallellibrary_amd import _C
    return [tuple(p) for p in _C.attn_block_order_host(n, bh).tolist()]


def _check(n, bh):
    got = _order(n, bh)
    assert sorted(got) == [(h, k) for h in range(bh) for k in range(n)]
    bh8 = bh & ~7
    for g in range(8):
        walk = [got[L] for L in range(g, n * bh8, 8)]
        assert walk == [(8 * t + g, k) for t in range(bh8 // 8)
                        for k in range(n)], (n, bh, g)
    for L in range(n * bh8, n * bh):
        assert got[L] == (L // n, L % n)


def test_every_small_grid():
    for n in range(1, 10):
        for bh in range(1, 42):
            _check(n, bh)


@pytest.mark.parametrize("n,bh", [(4, 2048), (1, 65535), (65535, 1),
                                  (65535, 9), (3, 4099)])
def test_large_grids(n, bh):
    _check(n, bh)


def test_below_eight_heads_is_identity():
    for n in (1, 4):
        for bh in range(1, 8):
            assert _order(n, bh) == [(y, x) for y in range(bh)
                                     for x in range(n)]
