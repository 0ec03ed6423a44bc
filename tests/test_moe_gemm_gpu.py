"""The grouped expert GEMMs (csrc/kernels/moe_gemm.hip) through _C, against
the fp64 product of the same bf16 inputs on the CPU.

Plain products: lm_head_cases.gemm_bound, E = gamma_k sum |a b| + V_BF16 |C|
with k the length of the contraction (the live rows for tn), judged at 2 E.
Dead input rows and the output buffers start as NaN: a dead row that is
read, or an output element that is not written, fails the NaN check; dead
output rows and tn of an empty expert must be exactly zero.

Epilogues, with u = U_F32, s the exact product and E_acc its accumulation
bound gamma_k sum |a b|.  The kernels use erff and expf, taken at the OpenCL
limits the device library meets (erf 16 ulp, exp 3 ulp):

* 1 + erf(x / sqrt 2): the argument carries two roundings (constant,
  product), which erf' <= 2 / sqrt(pi) and |t| exp(-t^2) < 1/2 turn into
  less than 1 u absolute; erf itself 16 u (|erf| <= 1); the sum 2 u.
  Absolute error <= 19 u, also where the sum cancels.
* act = bf16(gelu(acc)), gelu(x) = x/2 (1 + erf): gelu is 1.13-Lipschitz,
  so the accumulator contributes 1.13 E_acc; the erf factor 19/2 u |s|,
  the two products 2 u |gelu(s)|, the rounding V_BF16 |gelu(s)|:
  E = 1.13 E_acc + u (10 |s| + 2 |gelu s|) + V_BF16 |gelu s|.
* C = bf16(acc gelu'(pre)), gelu'(x) = (1 + erf)/2 + x c exp(-x^2/2),
  c = 1/sqrt(2 pi), of the SAME bf16 pre in the reference: the first term
  10 u; the second is at most 0.242 with relative error (6 + x^2/2) u
  (constant, two products, exp's 3 ulp, the rounded x^2 in the exponent),
  below 2 u absolute since x^3 exp(-x^2/2) c / 2 < 0.24; the sum 1.2 u.
  So |d' - d| <= 16 u with d = gelu'(pre) <= 1.13, and
  E = |d| E_acc + u (16 |s| + |s d|) + V_BF16 |s d|.
Second-order terms are left to the factor 2 of the judgement."""

import math

import pytest
import torch

from tests import kernel_refs as kr
from tests.lm_head_cases import F64, gemm_bound

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from easyparallellibrary_amd import _C
else:
    _C = None

E = 3
BM = 128                       # the kernels' row tile
MS = (1, BM - 1, BM + 1, 2 * BM + 7)
WIDTHS = (64, 192, 320)
PATTERNS = ("none", "mixed", "clamped")
NAN = float("nan")


def row_counts(pattern, m):
    """(rows given to the kernel, live rows per expert)"""
    if pattern == "none":
        return None, [m] * E
    if pattern == "mixed":         # empty, full, strictly inside a tile
        r = [0, m, m // 2 + 1 if m > 1 else 1]
    else:                          # both clamps
        r = [m + 5, -1, 1]
    return r, [min(max(x, 0), m) for x in r]


def shapes(form, m, k, n):
    """shapes of a, b, c within one expert"""
    return {"nn": ((m, k), (k, n), (m, n)), "nt": ((m, n), (k, n), (m, k)),
            "tn": ((m, k), (m, n), (k, n))}[form]


def gelu64(x):
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return (0.5 * (1.0 + torch.special.erf(x / math.sqrt(2.0))) +
            x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


def make(form, m, k, n, pattern, seed=0):
    gen = torch.Generator().manual_seed(seed + 13 * m + 5 * k + n)
    sa, sb, sc = shapes(form, m, k, n)
    rows, live = row_counts(pattern, m)
    a = torch.randn(E, *sa, generator=gen).to(torch.bfloat16)
    b = (torch.randn(E, *sb, generator=gen) * 0.25).to(torch.bfloat16)
    pre = torch.randn(E, *sc, generator=gen).mul(2.0).to(torch.bfloat16)
    for e in range(E):
        a[e, live[e]:] = NAN
        if form == "tn":
            b[e, live[e]:] = NAN
        if form == "nt":
            pre[e, live[e]:] = NAN
    rows_t = None if rows is None else torch.tensor(
        rows, dtype=torch.int32, device="cuda")
    return a, b, pre, rows_t, live, sc


def product(form, a, b, e, me):
    """fp64 reference and accumulation bound of expert e's live part"""
    a64, b64 = a[e].to(F64), b[e].to(F64)
    if form == "nn":
        x, y, kk = a64[:me], b64, a64.shape[1]
    elif form == "nt":
        x, y, kk = a64[:me], b64.t(), a64.shape[1]
    else:
        x, y, kk = a64[:me].t(), b64[:me], max(me, 1)
    ref, bound = gemm_bound(x, y, kk, True)
    return ref, bound, bound - kr.V_BF16 * ref.abs()


def judge(name, got, ref, bound, me, dead_rows):
    got = got.cpu()
    assert not torch.isnan(got).any(), name
    if dead_rows:
        assert torch.equal(got[me:], torch.zeros_like(got[me:])), name
        got = got[:me]
    err = (got.to(F64) - ref).abs()
    ratio = err / (2.0 * bound).clamp_min(1e-300)
    worst = ratio.max() if err.numel() else 0.0
    print("{}: worst err / 2E = {:.3f}".format(name, float(worst)))
    assert not (err > 2.0 * bound).any(), name


def run(form, a, b, rows, sc, aux=None):
    c = torch.full((E,) + sc, NAN, dtype=torch.bfloat16, device="cuda")
    fn = getattr(_C, "moe_gemm_" + form)
    if form == "tn":
        fn(c, a, b, rows)
    else:
        fn(c, a, b, rows, aux)
    return c


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("form", ("nn", "nt", "tn"))
def test_against_fp64(form, m, k, n, pattern):
    a, b, pre, rows, live, sc = make(form, m, k, n, pattern)
    ad, bd = a.cuda(), b.cuda()
    c = run(form, ad, bd, rows, sc)
    act = pre_d = c2 = None
    if form == "nn":
        act = torch.full_like(c, NAN)
        c2 = run(form, ad, bd, rows, sc, act)
        assert torch.equal(c2, c)          # the pre-activation is unchanged
    elif form == "nt":
        pre_d = pre.cuda()
        c2 = run(form, ad, bd, rows, sc, pre_d)
    torch.cuda.synchronize()
    for e in range(E):
        me = live[e]
        ref, bound, e_acc = product(form, a, b, e, me)
        tag = "{} e{} m_e {}".format(form, e, me)
        dead = form != "tn"
        if form == "tn" and me == 0:
            assert torch.equal(c[e].cpu(), torch.zeros(sc).to(c.dtype)), tag
        judge(tag, c[e], ref, bound, me, dead)
        if form == "nn":
            g = gelu64(ref)
            e_act = (1.13 * e_acc + kr.U_F32 * (10 * ref.abs() + 2 * g.abs())
                     + kr.V_BF16 * g.abs())
            judge(tag + " act", act[e], g, e_act, me, dead)
        elif form == "nt":
            d = dgelu64(pre[e, :me].to(F64))
            sd = ref * d
            e_pre = (d.abs() * e_acc + kr.U_F32 * (16 * ref.abs() + sd.abs())
                     + kr.V_BF16 * sd.abs())
            judge(tag + " pre", c2[e], sd, e_pre, me, dead)


@pytest.mark.parametrize("form", ("nn", "nt", "tn"))
def test_two_runs_agree_bitwise(form):
    a, b, pre, rows, _, sc = make(form, 2 * BM + 7, 320, 192, "mixed")
    ad, bd = a.cuda(), b.cuda()
    first, second = (run(form, ad, bd, rows, sc) for _ in range(2))
    torch.cuda.synchronize()
    assert torch.equal(first, second)


def test_bindings_refuse():
    def t(*shape):
        return torch.zeros(shape, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="multiples of 64"):
        _C.moe_gemm_nn(t(E, 8, 64), t(E, 8, 72), t(E, 72, 64))
    a, b, c = t(E, 8, 64), t(E, 64, 64), t(E, 8, 64)
    with pytest.raises(RuntimeError, match="device"):
        _C.moe_gemm_nn(c, a, b, torch.zeros(E, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="int32"):
        _C.moe_gemm_tn(t(E, 64, 64), a, c,
                       torch.zeros(E, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
