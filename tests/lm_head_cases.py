"""Cases, references and bounds shared by test_lm_head_live_rows_cpu.py and
test_lm_head_live_rows_gpu.py (no test in here).

Bound of a GEMM C = A B with fp32 accumulation over K terms, against the
fp64 product of the same inputs (conventions of tests/kernel_refs.py):
every order of summing K fp32 products is within gamma_K sum |a b| of the
exact sum (kr.gamma_k; padding rows add exact zeros, so K is the number of
rows of the full operand on every path), and a bf16 result is rounded
once more, V_BF16 |C|.  As for every bf16 tensor there, the kernels are
judged at 2 E (V_BF16 is half the unit roundoff of bf16); fp32 results at
1 E."""

import torch

from tests import kernel_refs as kr

F64 = torch.float64
NS = (1, 7, 256, 257, 1000)
VS = (8, 1000, 1032)
H = 64
MASKS = ("all_dead", "all_live", "first", "last", "mixed")


def live_mask(name, n):
    """bool [n]: the rows that get non-zero content"""
    live = torch.zeros(n, dtype=torch.bool)
    if name == "all_live":
        live[:] = True
    elif name == "first":
        live[0] = True
    elif name == "last":
        live[n - 1] = True
    elif name == "mixed":
        # about 15 %, neither end at n >= 7 so that "first" / "last" differ
        live[(torch.arange(n) * 2654435761 % 100) < 15] = True
        live[0] = False
        if n >= 4:
            live[3] = True
        if n >= 300:
            live[255:258] = torch.tensor([True, False, True])
    else:
        assert name == "all_dead"
    return live


def grad_matrix(name, n, v, dtype, specials=True, seed=0):
    """g [n, v] in ``dtype`` (CPU): randn on the live rows of live_mask,
    zero elsewhere.  With ``specials`` (mixed only, rows permitting): a
    live row whose single non-zero is its LAST element, a row of -0.0 only
    (dead) and a row holding one NaN (live).  Returns (g, live bool [n])."""
    gen = torch.Generator().manual_seed(seed + 7 * n + v)
    live = live_mask(name, n)
    g = torch.randn(n, v, generator=gen)
    g[g == 0] = 1.0
    g[~live] = 0.0
    if specials and name == "mixed" and n >= 7:
        g[1] = 0.0
        g[1, v - 1] = 0.5        # single non-zero, last element
        live[1] = True
        g[2] = -0.0              # dead
        live[2] = False
        g[5] = 0.0
        g[5, v // 2] = float("nan")
        live[5] = True
    return g.to(dtype), live


def gemm_bound(a, b, k, bf16):
    """E for C = a b (fp64 operands holding the kernel's inputs)"""
    ref = a @ b
    e = kr.gamma_k(k) * (a.abs() @ b.abs())
    e = e + (kr.V_BF16 if bf16 else kr.U_F32) * ref.abs()
    return ref, e


def head_refs(x, w, g, bf16):
    """fp64 (dx, dw) of y = x w^T under the gradient g, with bounds"""
    x64, w64, g64 = x.to(F64).cpu(), w.to(F64).cpu(), g.to(F64).cpu()
    dx, e_dx = gemm_bound(g64, w64, w64.shape[0], bf16)
    dw, e_dw = gemm_bound(g64.t(), x64, x64.shape[0], bf16)
    return dict(dx=dx, dw=dw, e_dx=e_dx, e_dw=e_dw)


def head_inputs(n, v, dtype, seed=0):
    gen = torch.Generator().manual_seed(1000 + seed + 3 * n + v)
    x = torch.randn(n, H, generator=gen).to(dtype)
    w = (torch.randn(v, H, generator=gen) * 0.5).to(dtype)
    return x, w


def bits(t):
    """the tensor's bit patterns as integers (NaN-safe equality)"""
    return t.contiguous().view(
        torch.int16 if t.element_size() == 2 else torch.int32)
