"""fp64 references, derived per-element rounding bounds and fp32
emulations for the LLaMA kernels (csrc/kernels/llama_ops.hip): RMSNorm
forward / backward, in-place RoPE and SwiGLU.

Built on kernel_refs.py (imported unchanged): the same input families, the
same criterion — |got - ref| <= 2 E on bf16 tensors, <= 1 E on fp32 ones
(rstd, dgamma), where E carries one bf16 rounding as v = 2^-9 (a correct
rounding alone reaches 1.992 E) and u = 2^-24 per fp32 operation.

Everything runs on the CPU in float64; test_llama_refs_cpu.py validates it
without a GPU (references against autograd, emulations within the bounds,
mutations far outside), the GPU tests compare the kernels against it.
"""

import math

import torch

from tests import kernel_refs as kr
from tests.kernel_refs import (F64, TINY_F32, U_F32, V_BF16,  # noqa: F401
                               GuardedBuffer, bf16_round, dy_family,
                               gamma_k, gelu_sweep, guarded_rows, ln_inputs,
                               ratio_of)

F32 = torch.float32
RMS_EPS = 1e-5
LOG2E = 1.4426950408889634

FACTOR = dict(out=2.0, s=2.0, dx=2.0, rstd=1.0, dgamma=1.0,      # RMSNorm
              y=2.0,                                              # RoPE
              dgate=2.0, dup=2.0)                                 # SwiGLU


def _rnd(t):
    return t.to(torch.bfloat16).to(F64)


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------
ROPE_B, ROPE_H = 2, 3
ROPE_DIMS = (64, 128)
ROPE_SEQS = (1, 33, 257)
ROPE_POS0 = (0, 4000)
ROPE_LAYOUTS = ("packed", "bhsd", "bshd", "padded")
ROPE_THETA = 10000.0


def rope_tables_ref(d, theta, length):
    """cos, sin [length, d/2]: fp64 angles pos * theta^(-i/(d/2)), rounded
    once to fp32 (returned as fp32 tensors)"""
    half = d // 2
    inv = torch.pow(torch.tensor(float(theta), dtype=F64),
                    -torch.arange(half, dtype=F64) / half)
    ang = torch.arange(length, dtype=F64)[:, None] * inv[None, :]
    return ang.cos().to(F32), ang.sin().to(F32)


def rope_ref(x, cos, sin, pos0, inverse=False):
    """x: fp64 [B, S, N, D]; cos, sin: the fp32 tables (inputs of the
    reference: their own rounding is not the kernel's).  Half-split:
    y1 = x1 c - x2 s, y2 = x2 c + x1 s; inverse flips the sign of s.
    Returns y and the magnitudes m = |x1 c| + |x2 s| (resp. |x2 c| +
    |x1 s|) the bound needs."""
    seq, d = x.shape[1], x.shape[3]
    half = d // 2
    c = cos[pos0:pos0 + seq].to(F64)[None, :, None, :]
    s = sin[pos0:pos0 + seq].to(F64)[None, :, None, :]
    if inverse:
        s = -s
    x1, x2 = x[..., :half], x[..., half:]
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    m = torch.cat([(x1 * c).abs() + (x2 * s).abs(),
                   (x2 * c).abs() + (x1 * s).abs()], dim=-1)
    return y, m


def rope_bounds(y, m):
    """two products and one add in fp32 (3u on the magnitudes; an FMA only
    drops one), then the single bf16 rounding"""
    return V_BF16 * y.abs() + (1 + V_BF16) * 3 * U_F32 * m


def rope_emulate(x, cos, sin, pos0, inverse=False):
    seq, d = x.shape[1], x.shape[3]
    half = d // 2
    c = cos[pos0:pos0 + seq][None, :, None, :]
    s = sin[pos0:pos0 + seq][None, :, None, :]
    if inverse:
        s = -s
    x1, x2 = x[..., :half].to(F32), x[..., half:].to(F32)
    return _rnd(torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1))


def rope_input(seq, d, n, seed=0, b=ROPE_B):
    """bf16-representable fp64 [b, seq, n, d], randn * 3"""
    gen = torch.Generator().manual_seed(seed + 7 * seq + d + 131 * n)
    return bf16_round(torch.randn(b, seq, n, d, generator=gen, dtype=F64) * 3)


def rope_cases():
    return [(d, seq, pos0) for d in ROPE_DIMS for seq in ROPE_SEQS
            for pos0 in ROPE_POS0]


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------
# 1536 is the one width with a 192-thread (three-wave) forward block
RMS_COLS = (8, 64, 504, 512, 520, 1024, 1536, 2048, 2056, 4096, 5120, 8192)
RMS_ROWS = (1, 3, 37)
RMS_GRID_CASES = ((64, 4099), (512, 8191))        # (cols, rows)
RMS_RSTD_REL_MAX = 2.0 ** -12


def rms_cases():
    return ([(c, r) for c in RMS_COLS for r in RMS_ROWS] +
            list(RMS_GRID_CASES))


# ---- the launch paths, as counts read from csrc/kernels/llama_ops.hip ------
def rms_fwd_path(cols):
    """rms_norm_fwd_kernel: block from rms_fwd_block, CHUNKS 1 / 2 / 4
    vectors of 8 columns per thread.  depth = additions on the longest
    path of the row sum: the thread's own addends, six butterfly steps,
    then the (waves - 1) posts added in order."""
    assert cols % 8 == 0 and 8 <= cols <= 8192
    need = cols // 8
    block = 64 if need <= 64 else 128 if need <= 128 else \
        192 if need <= 192 else 256
    chunks = 1 if cols <= 2048 else 2 if cols <= 4096 else 4
    if chunks > 1:
        block = 256
    return dict(block=block, chunks=chunks,
                depth=8 * chunks + 6 + (block // 64 - 1))


def rms_bwd_path(cols):
    """rms_norm_bwd_kernel: one row per wave up to 2048 columns (CHUNKS 1 /
    2 / 4, six butterfly steps), one row per 256-thread block above
    (CHUNKS 2 / 4, three more additions across the waves)"""
    assert cols % 8 == 0 and 8 <= cols <= 8192
    if cols <= 2048:
        chunks = 1 if cols <= 512 else 2 if cols <= 1024 else 4
        return dict(block=False, chunks=chunks, depth=8 * chunks + 6)
    chunks = 2 if cols <= 4096 else 4
    return dict(block=True, chunks=chunks, depth=8 * chunks + 9)


def rms_bwd_parts(rows, cols):
    """partial rows the backward writes, one per block
    (epl_rms_norm_bwd_parts)"""
    if cols <= 2048:
        return min((rows + 3) // 4, 1024)
    return min(rows, 1024)


def rms_ref(x, res, gamma, eps=RMS_EPS):
    s = x if res is None else x + res
    ms = (s * s).mean(dim=1)
    rstd = (ms + eps) ** -0.5
    return dict(s=s, ms=ms, rstd=rstd, out=s * rstd[:, None] * gamma)


def rms_fwd_bounds(ref, x, res, gamma, eps=RMS_EPS):
    """s   : the kernel forms s32 = fl32(x + res), one IEEE addition of
            exact inputs: e_s = |fl32(s) - s| is known exactly.  Stored
            once: v |s| + (1 + v) e_s.
    rstd: the mean of squares moves by mean(2 |s| e_s + e_s^2) through
            e_s; square, k-deep sum, division and + eps are gamma_{k+3}
            relative on ms (all addends >= 0: nothing cancels); eps itself
            is rounded to fp32 and cols converted (gamma_2).  With r the
            relative error of ms + eps, rsqrtf within 1 ulp (2u):
            rel = r / (2 (1 - r)) + 2u.
    out : s32 rstd^ gamma, two fp32 products (3u with the margin of one),
            s32 off by e_s, then the single bf16 rounding."""
    k = rms_fwd_path(x.shape[1])["depth"]
    u, v = U_F32, V_BF16
    s, ms, rstd = ref["s"], ref["ms"], ref["rstd"]
    e_s = (kr.f32_round(s) - s).abs()
    dms = (2 * s.abs() * e_s + e_s * e_s).mean(dim=1)
    r = (dms + gamma_k(k + 3) * ms) / (ms + eps) + gamma_k(2)
    rel = r / (2 * (1 - r)) + 2 * u
    out = ref["out"].abs()
    fp = out * (rel[:, None] + 3 * u) + gamma.abs() * rstd[:, None] * e_s
    return dict(rstd=rstd * rel, rel_rstd=rel,
                out=v * out + (1 + v) * fp,
                s=v * s.abs() + (1 + v) * e_s)


def rms_emulate(x, res, gamma, eps=RMS_EPS):
    s32 = x.to(F32) if res is None else x.to(F32) + res.to(F32)
    n = x.shape[1]
    rstd = torch.rsqrt((s32 * s32).sum(dim=1, keepdim=True) / n +
                       torch.tensor(eps, dtype=F32))
    return dict(rstd=rstd.squeeze(1).to(F64), s=_rnd(s32),
                out=_rnd(s32 * rstd * gamma.to(F32)))


def rms_bwd_ref(dy, s, gamma, rstd, dadd=None):
    """at the s / rstd the kernel is handed (exact inputs): xhat = s rstd,
    B = sum dy gamma xhat, o = rstd (dy gamma - xhat B / n), dx = o +
    dadd, dgamma = sum_rows dy xhat"""
    n = s.shape[1]
    xhat = s * rstd[:, None]
    dyg = dy * gamma
    b = (dyg * xhat).sum(dim=1, keepdim=True)
    o = (dyg - xhat * b / n) * rstd[:, None]
    dx = o if dadd is None else o + dadd
    return dict(xhat=xhat, dyg=dyg, b=b, o=o, dx=dx,
                dgamma=(dy * xhat).sum(dim=0))


def rms_bwd_bounds(ref, dy, s, gamma, rstd, dadd):
    """ln_bwd_bounds without the A term.  xhat^ = fl(s rstd): u |xhat|.
    dyg exact (bf16 x bf16).  B^: gamma_{k+3} sum |dyg xhat|.  o = (dyg -
    xhat (B fl(1/n))) rstd: xhat, 1/n and the two products are 4u on
    |xhat B| / n, the subtraction stays inside 4u (|dyg| + |xhat B| / n),
    the last product u |o|; adding dadd: u |o + dadd|.  dx is rounded
    once.  dgamma: R fp32 addends in any order, each carrying 3u."""
    n, rows = s.shape[1], s.shape[0]
    k = rms_bwd_path(n)["depth"]
    u, v = U_F32, V_BF16
    xhat, dyg, b = ref["xhat"], ref["dyg"], ref["b"]
    e_b = gamma_k(k + 3) * (dyg * xhat).abs().sum(dim=1, keepdim=True)
    xb = (xhat * b).abs()
    e_o = (rstd[:, None] * (xhat.abs() * e_b / n +
                            4 * u * (dyg.abs() + xb / n)) +
           u * ref["o"].abs())
    if dadd is not None:
        e_o = e_o + u * ref["dx"].abs()
    return dict(dx=v * ref["dx"].abs() + (1 + v) * e_o,
                dgamma=(gamma_k(rows) + 3 * u) *
                (dy * xhat).abs().sum(dim=0))


def rms_bwd_emulate(dy, s, gamma, rstd, dadd):
    n = s.shape[1]
    r32 = rstd.to(F32)[:, None]
    xhat = s.to(F32) * r32
    dyg = dy.to(F32) * gamma.to(F32)
    b = (dyg * xhat).sum(dim=1, keepdim=True)
    coef = b * (torch.tensor(1.0, dtype=F32) / n)
    o = (dyg - xhat * coef) * r32
    if dadd is not None:
        o = o + dadd.to(F32)
    return dict(dx=_rnd(o), dgamma=(dy.to(F32) * xhat).sum(dim=0).to(F64))


def rms_check_case(cols, rows, fwd_fn, bwd_fn):
    """One (cols, rows) case of the RMSNorm matrix through
    ``fwd_fn(inp, with_res) -> dict(rstd, out[, s])`` and
    ``bwd_fn(inp, dy, s_used, rstd, dadd) -> dict(dx, dgamma)`` (fp64
    results): forward with and without a residual over every rotation of
    the LN row kinds, then the backward at the forward's own s / rstd,
    with and without dadd, for the dy families of the shape.  Returns
    (worst, bad) as kr.ln_check_case does."""
    worst, bad = {}, []

    def note(name, family, r, label):
        slot = worst.setdefault(name, {})
        slot[family] = max(slot.get(family, 0.0), r)
        if not r <= FACTOR[name]:
            bad.append("{} {} {}: err/E {:.3g} > {}".format(
                label, name, family, r, FACTOR[name]))

    fams = [kind[1] for kind in kr.LN_KINDS]
    for rot in kr.ln_rots(rows):
        for with_res in (False, True):
            inp = ln_inputs(rows, cols, with_res, rot=rot)
            label = "res%d rot%d" % (with_res, rot)
            ref = rms_ref(inp["x"], inp["res"], inp["gamma"])
            e = rms_fwd_bounds(ref, inp["x"], inp["res"], inp["gamma"])
            assert float(e["rel_rstd"].max()) <= RMS_RSTD_REL_MAX
            got = fwd_fn(inp, with_res)
            names = ("rstd", "out") + (("s",) if with_res else ())
            for k in sorted(set(inp["kinds"].tolist())):
                sel = inp["kinds"] == k
                for name in names:
                    note(name, fams[k], ratio_of(
                        got[name][sel], ref[name][sel], e[name][sel]), label)
            if not all(bool(torch.isfinite(got[n]).all()) for n in names):
                bad.append(label + " forward not finite")
                continue
            s_used = got["s"] if with_res else inp["x"]
            for dy_name in kr.ln_dy_names(rows, rot):
                gen = torch.Generator().manual_seed(rot + 5 * cols + rows)
                dy = dy_family(dy_name, rows, cols, gen)
                for dadd in (None, inp["dadd"]):
                    r = rms_bwd_ref(dy, s_used, inp["gamma"], got["rstd"],
                                    dadd)
                    eb = rms_bwd_bounds(r, dy, s_used, inp["gamma"],
                                        got["rstd"], dadd)
                    res = bwd_fn(inp, dy, s_used, got["rstd"], dadd)
                    lab = "%s %s dadd%d" % (label, dy_name, dadd is not None)
                    for name in ("dx", "dgamma"):
                        note(name, dy_name, ratio_of(res[name], r[name],
                                                     eb[name]), lab)
                        if not bool(torch.isfinite(res[name]).all()):
                            bad.append(lab + " " + name + " not finite")
    return worst, bad


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------
SWIGLU_F = (8, 24, 512, 520, 4096, 11008)
SWIGLU_ROWS = (1, 3, 37, 1025)
SWIGLU_EXTREMES = (88.0, 89.0, 100.0, 127.0, 128.0, 130.0)
# the launcher's cap: 2048 blocks of 256 threads, one 8-column vector each
SWIGLU_GRID_THREADS = 2048 * 256


def swiglu_cases():
    return [(r, f) for f in SWIGLU_F for r in SWIGLU_ROWS]


def swiglu_passes(rows, f):
    """row passes of one launch: rows per pass = threads // (F / 8)"""
    vpr = f // 8
    blocks = max(min((rows * vpr + 255) // 256, 2048), (vpr + 255) // 256)
    rpp = blocks * 256 // vpr
    return (rows + rpp - 1) // rpp


def swiglu_sweep():
    """gelu_sweep() (every bf16 value of 2^-6 <= |g| <= 12, 0, +-40) plus
    +-88 .. +-130, ascending: past the overflow of 2^w and the flushed
    tail of the sigmoid on either side"""
    ext = torch.tensor(SWIGLU_EXTREMES, dtype=F64)
    return torch.cat([gelu_sweep(), ext, -ext]).sort().values


def swiglu_inputs(rows, f, seed=0):
    """gu [rows, 2F], dy [rows, F], bf16-representable fp64.  randn (gate
    scaled by 2), the leading gate elements replaced by the sweep — all of
    it when it fits, else evenly spaced points of it with both ends."""
    gen = torch.Generator().manual_seed(seed + 17 * rows + 4099 * f)
    g = bf16_round(torch.randn(rows, f, generator=gen, dtype=F64) * 2)
    up = bf16_round(torch.randn(rows, f, generator=gen, dtype=F64))
    dy = bf16_round(torch.randn(rows, f, generator=gen, dtype=F64))
    sweep = swiglu_sweep()
    m = min(sweep.numel(), rows * f)
    pick = torch.linspace(0, sweep.numel() - 1, m).round().long()
    g.reshape(-1)[:m] = sweep[pick]
    return dict(gu=torch.cat([g, up], dim=1), dy=dy, nsweep=m)


def swiglu_ref(gu, dy):
    f = gu.shape[1] // 2
    g, up = gu[:, :f], gu[:, f:]
    s = torch.sigmoid(g)
    d = s + g * s * (1 - s)
    return dict(g=g, up=up, s=s, D=d, out=g * s * up, dgate=dy * up * d,
                dup=dy * g * s)


def swiglu_bounds(ref, dy):
    """s = rcp(1 + exp2(g c)), c = fl(-log2 e): w = g c carries 2u |w| (the
    constant and the product), 2^w turns that into ln2 2u |w| relative and
    v_exp_f32 adds 2u; 1 + e inherits it scaled by e / (1 + e) = 1 - s,
    plus u; v_rcp_f32 2u more:
        rel_s = (1 - s)(ln2 2u |g log2 e| + 2u) + 3u.
    A value under the fp32 normal range may flush: TINY absolute on s.
    out  = (g s) u: |out| (rel_s + 2u) + |g up| TINY, rounded once.
    D    = s + g s (1 - s); 1 - s is off by s rel_s + u (1 - s):
        E_D = s rel_s + |g s| (s rel_s + u (1 - s)) + |g s (1 - s)| (rel_s
              + 3u) + u |D| + (1 + |g|) TINY
    dgate = (dy up) D (dy up exact): |dy up| E_D + 2u |dgate|;
    dup   = (dy g) s: |dup| (rel_s + 2u) + |dy g| TINY.  Each rounded
    once."""
    u, v, t = U_F32, V_BF16, TINY_F32
    g, up, s, d = ref["g"], ref["up"], ref["s"], ref["D"]
    rel_s = (1 - s) * (math.log(2.0) * 2 * u * (g * LOG2E).abs() + 2 * u) \
        + 3 * u
    out, dgate, dup = ref["out"].abs(), ref["dgate"].abs(), ref["dup"].abs()
    e_out = v * out + (1 + v) * (out * (rel_s + 2 * u) +
                                 (g * up).abs() * t + t)
    e_d = (s * rel_s + (g * s).abs() * (s * rel_s + u * (1 - s)) +
           (g * s * (1 - s)).abs() * (rel_s + 3 * u) + u * d.abs() +
           (1 + g.abs()) * t)
    e_dg = v * dgate + (1 + v) * ((dy * up).abs() * e_d + 2 * u * dgate + t)
    e_du = v * dup + (1 + v) * (dup * (rel_s + 2 * u) +
                                (dy * g).abs() * t + t)
    return dict(out=e_out, dgate=e_dg, dup=e_du)


def swiglu_emulate(gu, dy):
    f = gu.shape[1] // 2
    g, up, d = gu[:, :f].to(F32), gu[:, f:].to(F32), dy.to(F32)
    s = 1.0 / (1.0 + torch.exp2(g * torch.tensor(-LOG2E, dtype=F32)))
    gs = g * s
    return dict(out=_rnd(gs * up), dgate=_rnd((d * up) * (s + gs * (1.0 - s))),
                dup=_rnd((d * g) * s))


def swiglu_check_case(rows, f, fn):
    """``fn(inp) -> dict(out, dgate, dup)`` (fp64) against the reference"""
    inp = swiglu_inputs(rows, f)
    ref = swiglu_ref(inp["gu"], inp["dy"])
    e = swiglu_bounds(ref, inp["dy"])
    got = fn(inp)
    worst, bad = {}, []
    for name in ("out", "dgate", "dup"):
        r = ratio_of(got[name], ref[name], e[name])
        worst[name] = r
        if not r <= FACTOR[name]:
            bad.append("{}: err/E {:.3g} > {}".format(name, r, FACTOR[name]))
        if not bool(torch.isfinite(got[name]).all()):
            bad.append(name + " not finite")
    return worst, bad


def format_ratios(worst):
    return " ".join("{}={:.3f}".format(k, v) for k, v in sorted(worst.items()))
