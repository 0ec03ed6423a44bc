"""fp64 reference, per-element rounding bounds, an fp32 emulation and the
input families for the fused MoE router (csrc/kernels/moe_router.hip; the
semantics are those of easyparallellibrary_amd/ops/moe.py's docstring).

The reference is written by explicit formulas, forward and backward, with
no autograd; test_moe_router_refs_cpu.py validates it (against torch fp64
autograd, against the emulation, against mutated "wrong kernels") without
a GPU, test_moe_router_gpu.py compares the kernels with it.

Bounds.  u = 2^-24 (fp32 unit roundoff), v = 2^-8 (bf16 unit roundoff: one rounding
to nearest of a is within v |a|),
gamma_k = k u / (1 - k u).  ASSUMPTION: expf and logf are accurate to 2 ulp,
i.e. a relative error of at most 4u.  Source: the HIP documentation's
"HIP math API" table of single-precision device functions lists both at 1
ulp; twice that is taken.  Results below 2^-126 may be flushed: every
bound on a probability carries an absolute 2^-126.

  lse   s = sum_e exp(z_e - m), m the exact row max.  Each addend is off
        by r_e = u |z_e - m| (the rounded argument) + 4u (expf), the sum of
        at most 8 terms per lane and 6 shuffle steps by gamma_14, so s is off
        by r_s = sum_e e_e r_e / s + gamma_14 relative.  logf adds
        4u |log s|, the final addition u |lse|:
          E_lse = r_s + 4u log s + u |lse|.
  p     p_e = expf(fl(z_e - lse^)): the argument is off by E_lse + u |z_e -
        lse|, expf by 4u: r_p = E_lse + u |z_e - lse| + 4u relative (taken
        as expm1), E_p = p r_p + 2^-126.
  w     k = 1: exactly 1.  k = 2: S = p_1 + p_2 is off by max r_p + u, the
        quotient by u: E_w = w (r_pj + max r_p + 2u) + 2^-125 / S.
  psum  any order of N fp32 additions is within gamma_N of the sum of the
        addends' magnitudes: E_psum = gamma_N (psum + sum_t E_p) + sum_t E_p.
  L_bal f_e = fl(c_e) / fl(N k): 2u.  P_e = psum_e / N: u and E_psum / N.
        Their product, the 8-level tree over the experts, the factor E:
        E_bal = E sum_e f_e (E_psum_e / N + P_e (gamma_8 + 5u)).
  L_z   lse^2 is off by 2 |lse| E_lse + E_lse^2 + u lse^2 per token, the sum
        by gamma_N, the division by u.
  dz    the backward is handed the forward's own lse (within E_lse), so p
        is as above.  With a = a_bal + a_sel:
          a_bal = g_bal E f_e / N, five operations: 5u |a_bal|;
          w_j off by w_j (r_pj + r_S + u), r_S = max r_p + u;
          dot = sum_j dw_j w_j: E_dot = sum_j |dw_j| w_j (r_pj + r_S + 3u);
          a_sel_j = (dw_j - dot) / S:
            E_sel = (E_dot + u (|dw_j| + |dot|)) / S + |a_sel_j| (r_S + 2u);
          E_a = E_abal + E_sel + u |a|;
          pa = sum_e p_e a_e:
            E_pa = sum_e (|p a| (r_p + u) + p E_a) + gamma_14 sum_e |p a|;
          t1 = p (a - pa): E_t1 = |t1| (r_p + 2u) + p (E_a + E_pa);
          t2 = g_z (2 / N) lse p: E_t2 = |t2| (4u + r_p) + |g_z 2 / N| p E_lse;
        fp = E_t1 + E_t2 + u |dz|, then ONE rounding to the logits' dtype:
          bf16 E_dz = v |dz| + (1 + v) fp, fp32 E_dz = fp
        (plus 2^-126 (1 + |a - pa| + |g_z 2 lse / N|) for flushed p).
  topi, counts: exact.
"""

import torch

from tests import kernel_refs as kr

F64 = torch.float64
U = kr.U_F32
V_BF16 = kr.U_BF16       # one bf16 rounding to nearest: <= 2^-8 |a|
TINY = kr.TINY_F32
C_EXP = 4.0 * U          # assumed accuracy of expf / logf, relative

ROUTER_N = (1, 63, 64, 65, 1000)
ROUTER_E = (2, 8, 24, 64, 100, 256)
ROUTER_K = (1, 2)
ROUTER_DTYPES = (torch.bfloat16, torch.float32)
ROUTER_FAMILIES = ("randn", "shift1000", "spread90", "equal", "ties",
                   "never")
ROUTER_ALL_FAMILIES_N = 1000      # this N runs every family
ROUTER_GRID_STRIDE = (66601, 8)   # more tokens than one grid pass (65536)
# the cotangents of L_bal and L_z: fp32 values, as the kernel reads them
G_BAL = float(torch.tensor(0.7, dtype=torch.float32))
G_Z = float(torch.tensor(-1.3, dtype=torch.float32))
# allowed err / E, the project's convention (LN_FACTOR_*, ATTN_FACTOR)
ROUTER_FACTOR_F32 = 1.0
ROUTER_FACTOR_BF16_DZ = 2.0
MUTATIONS = ("tie_high", "f_after_capacity", "lse_nomax", "no_pa", "lse1")


def round_to(x, dtype):
    return x.to(torch.float32).to(dtype).to(F64)


def router_cases(n_experts, dtype=None):
    """(N, k, family) of the GPU matrix at one expert count: every N with
    one family in rotation, every family at N = 1000"""
    out = []
    rot = ROUTER_E.index(n_experts)
    for k in ROUTER_K:
        for i, n in enumerate(ROUTER_N):
            if n == ROUTER_ALL_FAMILIES_N:
                out += [(n, k, fam) for fam in ROUTER_FAMILIES]
            else:
                out.append((n, k, ROUTER_FAMILIES[
                    (i + rot + 3 * k) % len(ROUTER_FAMILIES)]))
    return out


def dead_expert(n_experts):
    return n_experts // 2


def router_logits(family, n, e, dtype, seed=0):
    """fp64 [n, e] logits whose values are representable in ``dtype``.

    randn     : standard normal.
    shift1000 : randn + 1000 (the max subtraction; in bf16 the spacing at
                1000 is 4, so whole rows tie).
    spread90  : uniform in (-90, 90): p underflows for some experts.
    equal     : every row constant (a different constant per row).
    ties      : randn; rows 0, 3, 6, .. get their largest value copied to
                another expert (a tie between 1st and 2nd), rows 1, 4, ..
                their second largest copied to another expert (2nd / 3rd,
                when e >= 3); the copy goes below or above the original
                index in turn.
    never     : randn with expert e // 2 at -30: never among the top two
                when e > 2, never first when e = 2.
    """
    gen = torch.Generator().manual_seed(
        seed + 7919 * ROUTER_FAMILIES.index(family) + 31 * n + e)
    z = torch.randn(n, e, generator=gen, dtype=F64)
    if family == "shift1000":
        z = z + 1000.0
    elif family == "spread90":
        z = torch.rand(n, e, generator=gen, dtype=F64) * 180.0 - 90.0
    elif family == "equal":
        z = z[:, :1].expand(n, e).clone()
    elif family == "never":
        z[:, dead_expert(e)] = -30.0
    z = round_to(z, dtype)
    if family == "ties":
        order = torch.sort(z, dim=1, descending=True, stable=True).indices
        for r in range(n):
            if r % 3 == 2 or (r % 3 == 1 and e < 3):
                continue
            src = int(order[r, r % 3])
            others = [j for j in order[r, 1 + r % 3:].tolist()]
            lower = [j for j in others if j < src]
            upper = [j for j in others if j > src]
            pick = lower if (r // 3) % 2 == 0 else upper
            pick = pick or lower or upper
            z[r, pick[0]] = z[r, src]
    return z


def router_dw(n, k, seed=0):
    gen = torch.Generator().manual_seed(seed + 17 * n + k)
    return torch.randn(n, k, generator=gen).to(F64)


def router_properties(z, k):
    """what the families are built to contain"""
    srt = torch.sort(z, dim=1, descending=True, stable=True)
    val = srt.values
    e = z.shape[1]
    lse = torch.logsumexp(z, dim=1)
    p32 = torch.exp(z - lse[:, None]).to(torch.float32)
    counts = torch.bincount(srt.indices[:, :k].reshape(-1), minlength=e)
    return dict(
        tie12=bool((val[:, 0] == val[:, 1]).any()),
        tie23=bool(e >= 3 and (val[:, 1] == val[:, min(2, e - 1)]).any()),
        empty_expert=bool((counts == 0).any()),
        underflow=bool((p32 == 0).any()),
        top3_distinct=bool(e < 3 or ((val[:, 0] != val[:, 1]) &
                                     (val[:, 1] != val[:, 2])).all()))


def capacity_of(n, k, e, factor=1.25):
    return max(1, int(factor * n * k / e))


def router_ref(z, k, dw=None, g_bal=0.0, g_z=0.0, mutate=None):
    """Forward and backward of the router in fp64 by explicit formulas.
    ``mutate`` names one of MUTATIONS: a wrong kernel."""
    assert z.dtype == F64
    n, e = z.shape
    if mutate == "lse_nomax":
        # fp32 arithmetic, or the overflow of exp would not show
        lse = z.to(torch.float32).exp().sum(dim=1).log().to(F64)
    else:
        m = z.max(dim=1).values
        s = torch.exp(z - m[:, None]).sum(dim=1)
        lse = m + torch.log(s)
    p = torch.exp(z - lse[:, None])
    if mutate == "tie_high":
        order = e - 1 - torch.sort(z.flip(1), dim=1, descending=True,
                                   stable=True).indices
    else:
        order = torch.sort(z, dim=1, descending=True, stable=True).indices
    topi = order[:, :k].contiguous()
    psel = p.gather(1, topi)
    ssel = psel.sum(dim=1)
    w = psel / ssel[:, None] if k > 1 else torch.ones_like(psel)
    counts = torch.bincount(topi.reshape(-1), minlength=e)
    fcounts = counts
    if mutate == "f_after_capacity":
        fcounts = counts.clamp(max=capacity_of(n, k, e))
    f = fcounts.to(F64) / float(n * k)
    psum = p.sum(dim=0)
    l_bal = e * (f * psum / n).sum()
    l_z = (lse * lse).sum() / n
    out = dict(lse=lse, p=p, topi=topi, topw=w, ssel=ssel, counts=counts,
               f=f, psum=psum, l_bal=l_bal, l_z=l_z)
    if dw is None:
        return out
    a_bal = (g_bal * e * f / n)[None, :].expand(n, e)
    a = a_bal.clone()
    a_sel = torch.zeros(n, k, dtype=F64)
    dot = torch.zeros(n, dtype=F64)
    if k > 1:
        dot = (dw * w).sum(dim=1)
        a_sel = (dw - dot[:, None]) / ssel[:, None]
        a.scatter_add_(1, topi, a_sel)
    pa = (p * a).sum(dim=1)
    if mutate == "no_pa":
        pa = torch.zeros_like(pa)
    zfac = lse if mutate == "lse1" else 2.0 * lse
    t1 = p * (a - pa[:, None])
    t2 = g_z * (zfac / n)[:, None] * p
    out.update(a_bal=a_bal, a=a, a_sel=a_sel, dot=dot, pa=pa, t1=t1, t2=t2,
               dz=t1 + t2, dw=dw, g_bal=g_bal, g_z=g_z)
    return out


def router_bounds(ref, z, k, dtype):
    """Per-element bounds of the kernels' outputs against router_ref (see
    the module docstring); ``ref`` has to hold the backward."""
    n, e = z.shape
    u = U
    lse, p = ref["lse"], ref["p"]
    m = z.max(dim=1).values
    ee = torch.exp(z - m[:, None])
    s = ee.sum(dim=1)
    r_s = (ee * (u * (z - m[:, None]).abs() + C_EXP)).sum(dim=1) / s + \
        kr.gamma_k(14)
    e_lse = r_s + C_EXP * torch.log(s) + u * lse.abs()
    r_p = torch.expm1(e_lse[:, None] + u * (z - lse[:, None]).abs() + C_EXP)
    e_p = p * r_p + TINY
    topi = ref["topi"]
    r_sel = r_p.gather(1, topi)
    r_max = r_sel.max(dim=1).values
    if k > 1:
        e_w = (ref["topw"] * (r_sel + r_max[:, None] + 2 * u) +
               2 * TINY / ref["ssel"][:, None])
    else:
        e_w = torch.zeros(n, k, dtype=F64)
    gn = kr.gamma_k(n)
    e_psum = gn * (ref["psum"] + e_p.sum(dim=0)) + e_p.sum(dim=0)
    f = ref["f"]
    e_bal = e * (f * (e_psum / n + ref["psum"] / n *
                      (kr.gamma_k(8) + 5 * u))).sum()
    sq = 2 * lse.abs() * e_lse + e_lse ** 2 + u * lse ** 2
    e_lz = (sq.sum() + gn * (lse ** 2 + sq).sum()) / n + u * ref["l_z"].abs()
    out = dict(lse=e_lse, topw=e_w, psum=e_psum, l_bal=e_bal, l_z=e_lz)
    if "dz" not in ref:
        return out
    a, pa, dw = ref["a"], ref["pa"], ref["dw"]
    e_a = 5 * u * ref["a_bal"].abs() + u * a.abs()
    if k > 1:
        r_ssel = r_max + u
        w = ref["topw"]
        e_dot = (dw.abs() * w * (r_sel + r_ssel[:, None] + 3 * u)).sum(dim=1)
        e_sel = ((e_dot[:, None] + u * (dw.abs() + ref["dot"].abs()[:, None]))
                 / ref["ssel"][:, None] +
                 ref["a_sel"].abs() * (r_ssel[:, None] + 2 * u))
        e_a = e_a.scatter_add(1, topi, e_sel)
    pam = (p * a).abs()
    e_pa = ((pam * (r_p + u) + p * e_a).sum(dim=1) +
            kr.gamma_k(14) * pam.sum(dim=1))
    e_t1 = ref["t1"].abs() * (r_p + 2 * u) + p * (e_a + e_pa[:, None])
    gz2 = abs(ref["g_z"]) * 2.0 / n
    e_t2 = ref["t2"].abs() * (4 * u + r_p) + gz2 * p * e_lse[:, None]
    fp = (e_t1 + e_t2 + u * ref["dz"].abs() +
          TINY * (1 + (a - pa[:, None]).abs() + gz2 * lse.abs()[:, None]))
    if dtype == torch.bfloat16:
        out["dz"] = V_BF16 * ref["dz"].abs() + (1 + V_BF16) * fp
    else:
        out["dz"] = fp
    return out


def router_emulate(z, k, dw, g_bal, g_z, dtype):
    """The kernels' arithmetic in torch fp32 ops, with their roundings:
    everything in fp32, dlogits rounded once to ``dtype``.  Selection is
    exact in the kernels, so it is taken from the fp64 values."""
    f32 = torch.float32
    n, e = z.shape
    zf = z.to(f32)
    assert bool((zf.to(F64) == z).all())
    m = zf.max(dim=1).values
    s = (zf - m[:, None]).exp().sum(dim=1)
    lse = m + s.log()
    p = (zf - lse[:, None]).exp()
    topi = torch.sort(z, dim=1, descending=True,
                      stable=True).indices[:, :k].contiguous()
    counts = torch.bincount(topi.reshape(-1), minlength=e)
    psel = p.gather(1, topi)
    ssel = psel.sum(dim=1)
    w = psel / ssel[:, None] if k > 1 else torch.ones_like(psel)
    psum = p.sum(dim=0)
    fn = torch.tensor(float(n), dtype=f32)
    f = counts.to(f32) / (fn * float(k))
    l_bal = float(e) * (f * (psum / fn)).sum()
    l_z = (lse * lse).sum() / fn
    gb = torch.tensor(g_bal, dtype=f32)
    gz2 = torch.tensor(g_z, dtype=f32) * (torch.tensor(2.0, dtype=f32) / fn)
    a = (gb * float(e) * f / fn)[None, :].expand(n, e).clone()
    if k > 1:
        dwf = dw.to(f32)
        dot = (dwf * w).sum(dim=1)
        a.scatter_add_(1, topi, (dwf - dot[:, None]) / ssel[:, None])
    pa = (p * a).sum(dim=1)
    d = p * (a - pa[:, None]) + (gz2 * lse)[:, None] * p
    return dict(lse=lse.to(F64), topi=topi, topw=w.to(F64), counts=counts,
                psum=psum.to(F64), l_bal=l_bal.to(F64), l_z=l_z.to(F64),
                dz=d.to(dtype).to(F64))


def router_ratios(got, ref, bounds):
    """worst err / bound per output; topi and counts: 0 when equal, inf
    otherwise"""
    out = {}
    for key in ("lse", "topw", "psum", "l_bal", "l_z", "dz"):
        if key in got and key in bounds:
            out[key] = kr.ratio_of(got[key].to(F64).reshape(ref[key].shape),
                                   ref[key], bounds[key])
    for key in ("topi", "counts"):
        if key in got:
            out[key] = 0.0 if torch.equal(got[key].cpu(), ref[key]) \
                else float("inf")
    return out


def router_allowed(dtype):
    fac = {key: ROUTER_FACTOR_F32
           for key in ("lse", "topw", "psum", "l_bal", "l_z", "dz")}
    if dtype == torch.bfloat16:
        fac["dz"] = ROUTER_FACTOR_BF16_DZ
    fac["topi"] = fac["counts"] = 0.0
    return fac
