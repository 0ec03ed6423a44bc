"""fp64 reference, derived rounding bounds, fp32 emulation and input
families for the fused AdamW step (csrc/kernels/kernels.hip:
fused_adamw_kernel), the squared-norm reduction and the bf16 rounding of
the arena utilities.

Everything here runs on the CPU and is validated without a GPU by
test_optim_refs_cpu.py; test_adamw_fp64_gpu.py and test_arena_utils_gpu.py
compare the kernels with it.

Hyper-parameters are fp32-representable doubles (f32(0.9), ...), given to
kernel and reference alike, so 1 - beta is exact in fp32 and both sides
compute the same operation.  u = 2^-24, gamma_k = k u / (1 - k u).

ASSUMPTION: sqrtf and the fp32 division are accurate to 2 ulp, a relative
error of at most 4u each.  Neither the ROCm headers nor the compiler's
option help state the device accuracy or the default of
-fhip-fp32-correctly-rounded-divide-sqrt, so the value the router bounds
take for expf is taken here too.  Results below 2^-126 may be flushed or
lose bits: every bound carries an absolute 2^-126.
"""

import math

import numpy as np
import torch

from tests.kernel_refs import (F64, TINY_F32, U_F32,  # noqa: F401
                               GuardedBuffer, LAMB_SHAPES, attn_flat,
                               attn_ratio, format_worst, gamma_k, ratio_of)

F32 = torch.float32
BF16 = torch.bfloat16


def f32(x):
    return float(torch.tensor(x, dtype=F32))


B1, B2, EPS, LR, WD = f32(0.9), f32(0.999), f32(1e-8), f32(1e-3), f32(0.01)
STEPS = (1, 2, 3, 5, 10, 1000, 100000)
C_SQRT = 4.0 * U_F32        # assumed accuracy of sqrtf, relative
C_DIV = 4.0 * U_F32         # assumed accuracy of the fp32 division
GRID_PASS = 8 * 256 * 4096  # elements of one pass of the capped grid
BIG_N = GRID_PASS + 13      # one vector past it, plus a tail of 5
SIZES = (7, 8, 12345, BIG_N)
SLICE = (1024, 128, 640)    # arena size, lo, hi


def inv_bias64(beta, step):
    return 1.0 / (1.0 - beta ** step)


def inv_bias_powf(beta, step):
    """the host arithmetic before the fix: fp32 powf, subtraction and
    division (numpy float32)"""
    one = np.float32(1.0)
    return float(one / (one - np.power(np.float32(beta), np.float32(step))))


def bf16_rne(x):
    """fp64 / fp32 tensor -> bf16, round to nearest even of the fp32 value
    (a second rounding only when x is fp64 and not an fp32)"""
    return x.to(F32).to(BF16)


def bf16_half_step(x):
    """half the bf16 spacing at |x| (fp64): 2^(e - 8) for 2^e <= |x|"""
    ax = x.abs().clamp_min(TINY_F32)
    return 2.0 ** (torch.floor(torch.log2(ax)) - 8)


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
def adamw_ref(master, grad, m, v, lr, beta1, beta2, eps, weight_decay, step,
              inv_scale):
    """One AdamW step by explicit fp64 formulas, FusedAdamW._step_torch's
    definition.  master, grad, m, v: fp64 flat tensors (not modified).
    Returns m, v, the update u = mhat / (sqrt(vhat) + eps), master
    = p - lr (u + wd p), param = RNE bf16 of that master, and the
    intermediates the bounds are built from."""
    assert all(t.dtype == F64 for t in (master, grad, m, v))
    g = grad * inv_scale
    a = beta1 * m
    b = (1.0 - beta1) * g
    m_new = a + b
    v_new = beta2 * v + (1.0 - beta2) * g * g
    ib1, ib2 = inv_bias64(beta1, step), inv_bias64(beta2, step)
    mhat = m_new * ib1
    vhat = v_new * ib2
    root = vhat.sqrt()
    update = mhat / (root + eps)
    decay = weight_decay * master
    new_master = master - lr * (update + decay)
    return dict(m=m_new, v=v_new, update=update, master=new_master,
                param=bf16_rne(new_master), a=a, b=b, mhat=mhat, vhat=vhat,
                root=root, decay=decay, ib1=ib1, ib2=ib2)


def adamw_bounds(ref, lr, eps):
    """Per-element E for m, v, update and master of the kernel

        g' = fl(g s)                 exact for a power-of-two s
        m' = fl(fl(b1 m) + fl(c1 g'))            c1 = 1 - b1, exact
        v' = fl(fl(b2 v) + fl(fl(c2 g') g'))     c2 = 1 - b2, exact
        q  = fl(fl(m' i1) / fl(sqrtf(fl(v' i2)) + eps))
        p' = fl(p - fl(lr fl(q + fl(wd p))))

    with i1, i2 one correctly rounded fp32 value each.  A contraction of
    a * b + c into an fma removes one rounding of a term and adds none, so
    every count below holds for any mix of fused and unfused forms.

    m   the b1 m term is rounded twice (product, sum), the g term three
        times (g', product, sum): E_m = gamma_3 (|b1 m| + |c1 g'|) + TINY,
        an absolute bound; it governs when the two terms cancel.
    v   every addend is positive.  g'^2 carries 2 roundings, the two
        products and the sum 3 more: E_v = gamma_5 v' + TINY; the floor
        covers g'^2 in the denormal range.
    q   mhat: E_mh = i1 E_m (1 + gamma_2) + gamma_2 |mhat| (i1's rounding
        and the product's).  vhat: E_vh = i2 E_v (1 + gamma_2) + gamma_2
        vhat.  |sqrt x - sqrt y| = |x - y| / (sqrt x + sqrt y) is at most
        E_vh / sqrt(vhat) and at most sqrt(E_vh); the smaller is taken
        (the second one when vhat is 0 or denormal), then sqrtf's own
        C_SQRT and the sum's u: E_den.  The quotient:
        (E_mh + |q| E_den) / (den - E_den), the division's C_DIV on top:
        E_u.
    p'  t = q + wd p: E_u + gamma_2 (|q| + |wd p|) (the decay product and
        the sum), times lr with one more rounding: lr (E_u + gamma_3 (|q|
        + E_u + |wd p|)), and the final subtraction rounds the stored
        value: u (|p'| + that).  With lr = 0 the product is 0 and the
        subtraction exact: E = 0, master keeps its bits.
    """
    u, t = U_F32, TINY_F32
    g2, g3, g5 = gamma_k(2), gamma_k(3), gamma_k(5)
    e_m = g3 * (ref["a"].abs() + ref["b"].abs()) + t
    e_v = g5 * ref["v"] + t
    e_mh = ref["ib1"] * e_m * (1 + g2) + g2 * ref["mhat"].abs()
    e_vh = ref["ib2"] * e_v * (1 + g2) + g2 * ref["vhat"]
    root = ref["root"]
    e_root_in = torch.minimum(e_vh / root.clamp_min(1e-300), e_vh.sqrt())
    e_root = e_root_in + C_SQRT * (root + e_root_in) + t
    den = root + eps
    e_den = e_root + u * (den + e_root)
    assert bool((den > 2 * e_den).all())
    q = ref["update"].abs()
    e_q = (e_mh + q * e_den) / (den - e_den)
    e_u = e_q + C_DIV * (q + e_q) + t
    if lr == 0.0:
        e_p = torch.zeros_like(q)
    else:
        step = lr * (e_u + g3 * (q + e_u + ref["decay"].abs()))
        e_p = step + u * (ref["master"].abs() + step) + t
    return dict(m=e_m, v=e_v, update=e_u, master=e_p)


# ---------------------------------------------------------------------------
# fp32 emulation of the kernel's arithmetic
# ---------------------------------------------------------------------------
def _fma(a, b, c):
    """fl32(a b + c): the fp32 product is exact in fp64, the sum is rounded
    to 53 bits and then to 24 (a double rounding moves the result by at
    most u 2^-29 relative beyond the single one)"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def adamw_emulate(master, grad, m, v, lr, beta1, beta2, eps, weight_decay,
                  step, inv_scale, fused, inv_bias=None):
    """The kernel's arithmetic in torch fp32, one rounding per operation;
    ``fused`` contracts every a * b + c the expression has into an fma.
    master, m, v: fp32; grad: bf16 or fp32.  ``inv_bias`` overrides the
    (inv_bias1, inv_bias2) pair, for the host arithmetic under test."""
    def c(x):
        return torch.tensor(x, dtype=F32)
    b1, b2, c1, c2 = c(beta1), c(beta2), c(1.0) - c(beta1), c(1.0) - c(beta2)
    if inv_bias is None:
        inv_bias = (inv_bias64(beta1, step), inv_bias64(beta2, step))
    i1, i2 = c(inv_bias[0]), c(inv_bias[1])
    g = grad.to(F32) * c(inv_scale)
    if fused:
        m_new = _fma(b1, m, c1 * g)
        v_new = _fma(b2, v, (c2 * g) * g)
    else:
        m_new = b1 * m + c1 * g
        v_new = b2 * v + (c2 * g) * g
    q = (m_new * i1) / ((v_new * i2).sqrt() + c(eps))
    if fused:
        p = _fma(-c(lr), _fma(c(weight_decay), master, q), master)
    else:
        p = master - c(lr) * (q + c(weight_decay) * master)
    return dict(m=m_new, v=v_new, master=p, param=p.to(BF16))


# ---------------------------------------------------------------------------
# criterion
# ---------------------------------------------------------------------------
def same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.dtype.itemsize]
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def adamw_judge(got, ref, e, select=None):
    """err / E per output of ``got`` (fp32 m, v, master and, where the
    instantiation has one, the bf16 param) against the reference:
    1 x E on m, v, master; param_rne is 0 where param equals RNE of the
    kernel's own master bit for bit and inf otherwise; param is its
    distance from the reference master over half a bf16 step plus E.
    ``select``: a mask of the elements to judge."""
    def s(x):
        return x if select is None else x[select]
    out = {}
    for name in ("m", "v", "master"):
        out[name] = ratio_of(s(got[name].to(F64)), s(ref[name]), s(e[name]))
    if got.get("param") is not None:
        out["param_rne"] = 0.0 if same_bits(
            s(got["param"]), s(got["master"].to(BF16))) else float("inf")
        want = s(ref["master"])
        bound = bf16_half_step(want.abs() + s(e["master"])) + s(e["master"])
        out["param"] = ratio_of(s(got["param"].to(F64)), want, bound)
    return out


# ---------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------
# (family, variant): see adamw_inputs
CASES = (
    ("randn", ""), ("zero_master", "wd0"), ("zero_master", "wd"),
    ("small_master", ""), ("big_master", ""), ("cancel_m", ""),
    ("zero_grad", "live"), ("zero_grad", "all"), ("tiny_grad", ""),
    ("scaled", "2^-44"), ("scaled", "2^-16"), ("scaled", "third"))
INSTANCES = ((True, True), (False, True), (True, False), (False, False))


def case_name(case):
    return case[0] + ("_" + case[1] if case[1] else "")


def _prior_state(n, gen):
    """m, v after two reference steps from zero on randn gradients"""
    z = torch.zeros(n, dtype=F64)
    m, v = z, z
    for step in (1, 2):
        r = adamw_ref(z, torch.randn(n, generator=gen, dtype=F64), m, v,
                      LR, B1, B2, EPS, 0.0, step, 1.0)
        m, v = r["m"], r["v"]
    return m.to(F32), v.to(F32)


def adamw_inputs(case, n, grad_bf16, seed=0):
    """fp32 master, m, v, the gradient in its own dtype, weight decay and
    inv_scale of one family:

    randn         p, g ~ N(0,1), m and v from two prior reference steps
    zero_master   p = 0 (wd 0 and WD): p' = -lr u shows u to a few ulp
    small_master  p = 2^-20 randn
    big_master    |p| = 2^10, wd 0, m and g of 2^-8 randn against v = 1:
                  lr |u| stays below a quarter ulp, the bits must not move
    cancel_m      m = fl(-(1 - b1) / b1 g): m' is rounding noise
    zero_grad     g = 0 with a live state; g = m = v = 0 (u = 0)
    tiny_grad     g = 2^-70 randn, m = v = 0: g'^2 is denormal and
                  sqrt(vhat) << eps; p = 0 at the even elements
    scaled        g = 2^44 randn at inv_scale 2^-44, 2^16 at 2^-16, and
                  3 randn at the non-power-of-two f32(1/3)
    """
    family, variant = case
    gen = torch.Generator().manual_seed(1000 * seed + n % 997)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    m, v = _prior_state(n, gen)
    wd, inv_scale = WD, 1.0
    if family == "zero_master":
        p = torch.zeros(n)
        wd = 0.0 if variant == "wd0" else WD
    elif family == "small_master":
        p = p * 2.0 ** -20
    elif family == "big_master":
        p = torch.where(p < 0, -1.0, 1.0) * 2.0 ** 10
        g, m, v, wd = g * 2.0 ** -8, g.flip(0) * 2.0 ** -8, torch.ones(n), 0.0
    elif family == "zero_grad":
        g = torch.zeros(n)
        if variant == "all":
            m, v = torch.zeros(n), torch.zeros(n)
    elif family == "tiny_grad":
        g = g * 2.0 ** -70
        m, v = torch.zeros(n), torch.zeros(n)
        p[0::2] = 0
    elif family == "scaled":
        mul, inv_scale = {"2^-44": (2.0 ** 44, 2.0 ** -44),
                          "2^-16": (2.0 ** 16, 2.0 ** -16),
                          "third": (3.0, f32(1.0 / 3.0))}[variant]
        g = g * mul
    else:
        assert family in ("randn", "cancel_m"), family
    g = g.to(BF16 if grad_bf16 else F32)
    if family == "cancel_m":
        m = (g.to(F64) * (-(1.0 - B1) / B1)).to(F32)
        v = p.flip(0) ** 2
    return dict(master=p, grad=g, m=m, v=v, wd=wd, inv_scale=inv_scale)


def adamw_reference_of(inp, lr, step):
    """(ref, E) of one step from the state in ``inp`` (fp32 tensors, or the
    kernel's own previous state)"""
    ref = adamw_ref(inp["master"].to(F64), inp["grad"].to(F64),
                    inp["m"].to(F64), inp["v"].to(F64), lr, B1, B2, EPS,
                    inp["wd"], step, inp["inv_scale"])
    return ref, adamw_bounds(ref, lr, EPS)


def adamw_matrix():
    """(n or 'slice', case, step, lr, grad_bf16, with_param) of the GPU
    matrix: every family and step at 12345 (the instantiation and lr = 0
    in rotation), every instantiation with one family in rotation at the
    other sizes.  The 8.4M-element size is not in here: its one shared
    case is adamw_big_case()."""
    out, i = [], 0
    for case in CASES:
        for step in STEPS:
            out.append((12345, case, step, 0.0 if i % 5 == 4 else LR)
                       + INSTANCES[i % 4])
            i += 1
    for n in (7, 8, "slice"):
        for inst in INSTANCES:
            out.append((n, CASES[i % len(CASES)], STEPS[i % len(STEPS)], LR)
                       + inst)
            i += 1
    return out


BIG_CASE, BIG_STEP = ("randn", ""), 3


def adamw_big_case():
    """The one input set of the 8.4M-element size: its gradients are bf16
    values, so the four instantiations share one reference."""
    inp = adamw_inputs(BIG_CASE, BIG_N, True)
    ref, e = adamw_reference_of(inp, LR, BIG_STEP)
    keep = ("m", "v", "master")
    return inp, {k: ref[k] for k in keep}, {k: e[k] for k in keep}


# ---------------------------------------------------------------------------
# sqnorm
# ---------------------------------------------------------------------------
def sqnorm_ref(x, out0=0.0):
    return float((x.to(F64) ** 2).sum()) + out0


def sqnorm_launch(n):
    """(blocks, addends per thread) of epl_sqnorm: 256-thread blocks, at
    most 1024 of them, a grid-stride loop"""
    blocks = min(max((n + 255) // 256, 1), 1024)
    return blocks, -(-n // (blocks * 256))


def sqnorm_bounds(n, ref):
    """Every addend is non-negative, so the error is relative to the sum:
    gamma_K ref with K the roundings on the longest path to ``out``: the
    square (1), the thread's addends, the 8 steps of the block tree (6
    shuffles in the wave, 2 across the 4 waves) and one atomic add per
    block, in any order."""
    blocks, addends = sqnorm_launch(n)
    return gamma_k(1 + addends + 8 + blocks) * ref


# ---------------------------------------------------------------------------
# bf16 rounding of the arena kernels (f2bf), as bit models
# ---------------------------------------------------------------------------
NAN_PATTERNS = (0x7fffffff, 0xffffffff, 0x7fff8000, 0x7f800001)
LOW_HALVES = (0, 1, 0x7fff, 0x8000, 0x8001, 0xffff)


def f2bf_parent(bits):
    """the rounding add alone (uint32 numpy array -> uint16)"""
    x = bits.astype(np.uint64)
    lsb = (x >> 16) & 1
    return (((x + 0x7fff + lsb) & 0xffffffff) >> 16).astype(np.uint16)


def f2bf_fixed(bits):
    nan = (bits & 0x7fffffff) > 0x7f800000
    return np.where(nan, ((bits >> 16) | 0x40).astype(np.uint16),
                    f2bf_parent(bits))


def f32_from_bits(bits):
    """uint32 values (any integer sequence) -> fp32 tensor"""
    arr = np.asarray(bits, dtype=np.uint32)
    return torch.from_numpy(arr.view(np.int32).copy()).view(F32)


def bf16_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def all_bit_patterns():
    hi = np.arange(65536, dtype=np.uint32)[:, None] << 16
    return (hi | np.asarray(LOW_HALVES, dtype=np.uint32)[None, :]).reshape(-1)


def cast_edge_values():
    """fp32 values for the cast kernels: ties under an even and an odd high
    half, the largest finite value, denormals, +-0, +-Inf, the NaN
    patterns, padded with randn"""
    return [0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x7f7fffff,
            0xff7fffff, 0x00000001, 0x007fffff, 0x00008000, 0x80018000,
            0x00000000, 0x80000000, 0x7f800000, 0xff800000] + \
        list(NAN_PATTERNS)
