"""The four MoE dispatch / combine kernels (csrc/kernels/moe.hip) called
directly, against fp64 index-op references (tests/kernel_refs.py), with
assignment lists built from a deterministic expert choice so that the
hard cases are certainly there: over-capacity assignments, tokens that
keep one of two slots, tokens that keep none, an expert nobody chose.

hidden 8 / 512 / 520 / 1536: one active lane, exactly one pass of the
64-lane x 8 column loop, one pass plus one lane, three passes.  The
grid-stride cases (70000 tokens, hidden 8) take both the
assignment-indexed and the token-indexed kernels round their outer loop
(more rows than the 65536 waves of a full grid).

Outputs that a kernel must write completely start as NaN; outputs it must
write only at kept slots (disp, dh: the callers pre-zero them and rely on
the rest staying untouched) start as 7.0.

Bounds: dispatch forward is a copy (exact).  dispatch backward and dh are
one bf16 rounding of an fp32 value: 2**-8 |ref| (one bf16 ulp).  combine
forward: 2**-8 * sum_j |fw_j h_j|.  dfw: hidden * 2**-23 * sum_c
|dout_c h_c| (fp32 dot product, any order).
"""

import pytest
import torch

from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from easyparallellibrary_amd import _C
else:
    _C = None

F64 = torch.float64
E = 4
SENTINEL = 7.0
BF16_ULP = 2.0 ** -8


def dev():
    return torch.device("cuda:0")


def _cpu64(t):
    return t.detach().cpu().to(F64)


def _randn_bf16(gen, *shape):
    return torch.randn(*shape, generator=gen).to(torch.bfloat16)


def _run(pattern, k, cap, n_tokens, hidden, claims_name=None):
    fe, pos, ft, inv, fw = kr.moe_assignment(n_tokens, k, E, cap, pattern)
    # everything the kernels index with, against the buffers' extents
    if claims_name is not None:
        props = kr.moe_check_claims(claims_name, fe, pos, ft, inv, k, E,
                                    cap, n_tokens)
    else:
        kr.moe_check_lists(fe, pos, ft, inv, k, E, n_tokens)
        props = kr.moe_properties(fe, pos, ft, k, E, cap, n_tokens)
        assert props["dropped"] > 0
    assert hidden % 8 == 0 and cap >= 1
    keep = pos < cap
    m = fe.numel()
    assert m == n_tokens * k
    assert fw.dtype == torch.float32 and fw.numel() == m
    none_kept = props["kept_per_token"] == 0
    gen = torch.Generator().manual_seed(hidden * 31 + n_tokens + k)
    x = _randn_bf16(gen, n_tokens, hidden)
    ddisp = _randn_bf16(gen, E, cap, hidden)
    h = _randn_bf16(gen, E, cap, hidden)
    dout = _randn_bf16(gen, n_tokens, hidden)
    for t in (x, ddisp, h, dout):
        assert (t.float() != SENTINEL).all()
    d = dev()
    fe_d, pos_d, ft_d, inv_d, fw_d = (t.to(d) for t in
                                      (fe, pos, ft, inv, fw))

    # ---- dispatch forward: a pure copy into kept slots ------------------
    disp = torch.full((E, cap, hidden), SENTINEL, dtype=torch.bfloat16,
                      device=d)
    _C.moe_dispatch_fwd(disp, x.to(d), fe_d, pos_d, ft_d, cap)
    torch.cuda.synchronize()
    ref, written = kr.moe_dispatch_fwd_ref(x, fe, pos, ft, E, cap)
    assert int(written.sum()) == int(keep.sum())
    got = _cpu64(disp)
    assert torch.equal(got[written], ref[written])
    assert (got[~written] == SENTINEL).all()

    # ---- dispatch backward ----------------------------------------------
    dx = torch.full((n_tokens, hidden), float("nan"), dtype=torch.bfloat16,
                    device=d)
    _C.moe_dispatch_bwd(dx, ddisp.to(d), fe_d, pos_d, inv_d, k, cap)
    torch.cuda.synchronize()
    got = _cpu64(dx)
    ref = kr.moe_dispatch_bwd_ref(ddisp, fe, pos, ft, n_tokens, cap)
    assert not torch.isnan(got).any()
    assert (got[none_kept] == 0).all()
    err = (got - ref).abs()
    assert (err <= BF16_ULP * ref.abs()).all()
    e_dx = (err / ref.abs().clamp_min(1e-30)).max().item()

    # ---- combine forward --------------------------------------------------
    out = torch.full((n_tokens, hidden), float("nan"), dtype=torch.bfloat16,
                     device=d)
    _C.moe_combine_fwd(out, h.to(d), fw_d, fe_d, pos_d, inv_d, k, cap)
    torch.cuda.synchronize()
    got = _cpu64(out)
    ref, mag = kr.moe_combine_fwd_ref(h, fw, fe, pos, ft, n_tokens, cap)
    assert not torch.isnan(got).any()
    assert (got[none_kept] == 0).all()
    err = (got - ref).abs()
    assert (err <= BF16_ULP * mag).all(), (err / mag.clamp_min(1e-30)).max()
    e_out = (err / mag.clamp_min(1e-30)).max().item()

    # ---- combine backward -------------------------------------------------
    dh = torch.full((E, cap, hidden), SENTINEL, dtype=torch.bfloat16,
                    device=d)
    dfw = torch.full((m,), float("nan"), dtype=torch.float32, device=d)
    _C.moe_combine_bwd(dh, dfw, dout.to(d), h.to(d), fw_d, fe_d, pos_d,
                       ft_d, cap)
    torch.cuda.synchronize()
    ref_dh, ref_dfw, dmag = kr.moe_combine_bwd_ref(dout, h, fw, fe, pos, ft,
                                                   E, cap)
    got = _cpu64(dh)
    err = (got - ref_dh).abs()
    assert (err[written] <= BF16_ULP * ref_dh[written].abs()).all()
    assert (got[~written] == SENTINEL).all()
    got_dfw = _cpu64(dfw)
    assert not torch.isnan(got_dfw).any()
    assert (got_dfw[~keep] == 0).all()
    ferr = (got_dfw - ref_dfw).abs()
    ftol = hidden * 2.0 ** -23 * dmag
    assert (ferr <= ftol).all(), (ferr / ftol.clamp_min(1e-30)).max()
    print("%s k %d cap %d tokens %d hidden %d: kept %d of %d; max rel err "
          "dx %.3g, out/sum|fw h| %.3g (bounds %.3g), dfw err/bound %.3g"
          % (claims_name or pattern, k, cap, n_tokens, hidden,
             int(keep.sum()), m, e_dx, e_out, BF16_ULP,
             (ferr / ftol.clamp_min(1e-30))[keep].max().item()))


@pytest.mark.parametrize("hidden", [8, 512, 520, 1536])
@pytest.mark.parametrize("name", sorted(kr.MOE_PATTERNS))
def test_moe_kernels(name, hidden):
    pattern, k, cap = kr.MOE_PATTERNS[name]
    _run(pattern, k, cap, 96, hidden, claims_name=name)


@pytest.mark.parametrize("pattern,k,cap", [("uneven1", 1, 20000),
                                           ("skew", 2, 40000)])
def test_moe_grid_stride(pattern, k, cap):
    n_tokens = 70000
    assert n_tokens > 16384 * 4      # waves of the largest grid
    _run(pattern, k, cap, n_tokens, 8)
