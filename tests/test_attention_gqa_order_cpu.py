"""The group-aware block orders of the q-parallel GQA attention grids
(csrc/kernels/attn_block_order.h: block_of_group, causal_group_bh)
evaluated on the host: bijections onto [0, B*H) x [0, n), with a group's
blocks where the header says they are."""

import pytest

SMALL = [(n, bhkv, g) for n in (1, 2, 3, 5) for bhkv in range(1, 27)
         for g in (1, 2, 3, 4, 8)]


def _order(n, bhkv, g, causal):
    from easyparallellibrary_amd import _C
    return _C.attn_gqa_order_host(n, bhkv, g, causal).tolist()


@pytest.mark.parametrize("n,bhkv,g", SMALL + [(7, 4099, 4), (65535, 9, 1),
                                              (300, 16, 64)])
def test_non_causal_order(n, bhkv, g):
    got = [tuple(p) for p in _order(n, bhkv, g, False)]
    assert sorted(got) == [(bh, k) for bh in range(bhkv * g)
                           for k in range(n)]
    # the n * G blocks of a batch-kv-head follow each other on one XCD
    for c in range(8):
        walk = got[c:n * g * (bhkv & ~7):8]
        assert walk == [((8 * t + c) * g + j, k) for t in range(bhkv // 8)
                        for j in range(g) for k in range(n)]


@pytest.mark.parametrize("n,bhkv,g", [c for c in SMALL if c[0] == 1] +
                         [(1, 4099, 4), (1, 65535, 1), (1, 1023, 64)])
def test_causal_order(n, bhkv, g):
    got = _order(n, bhkv, g, True)
    assert sorted(got) == list(range(bhkv * g))
    lim = g * (bhkv & ~7)
    # below the limit the heads of one group share x % 8
    for x in range(lim):
        assert got[x] // g % 8 == x % 8
    assert got[lim:] == list(range(lim, bhkv * g))
