"""LM-head projection whose backward runs on the live rows only.

An MLM loss masks about 15 % of the positions, so 85 % of the rows of the
gradient that reaches the decoder (65536 x 30528 at the bench shape) are
exactly zero, and both backward GEMMs (dX = dY W, dW = dY^T X) mostly
multiply zeros.  ``LiveRowsLinear`` keeps the forward as it is (the same
``F.linear`` call, the same logits) and in the backward

1. finds the rows of dY that hold any element != 0 (``rows_live_index``:
   ascending, no atomics, count stays on the device),
2. reads the count on the host: the one sync, the GEMM shapes need it,
3. pads it to a multiple of 256 (few distinct GEMM shapes; pad rows are
   zero and add +0),
4. gathers dY and X into [n_pad, V] and [n_pad, H],
5. runs the two GEMMs on those,
6. scatters dX back, zero rows everywhere else.

This is exact for any loss: a zero row adds +0 to dW and gives a zero row
of dX.  The dense backward (the two GEMMs autograd issues for F.linear)
runs while a stream is capturing, for tensors the kernels do not take
(other dtypes, non-contiguous dY, rows that are no multiple of 16 bytes)
and when half the rows or more are live.  On the CPU the same steps run
with torch boolean indexing, so the path is testable without a GPU.

Kernels: csrc/kernels/kernels.hip (rows_flag / rows_scan / gather_rows /
scatter_rows_zero).  No reference counterpart.
"""

import os

import torch
import torch.nn.functional as F

from easyparallellibrary_amd.ops.dispatch import native_ext, use_native

PAD_ROWS = 256          # n_pad = count rounded up to this
DENSE_FRACTION = 0.5    # n_pad >= this share of N: the dense GEMMs run


def resolve_live_rows(flag):
    """The constructor switch under EPL_LMHEAD_LIVE_ROWS: "0" / "1" force
    it off / on for every head, anything else leaves the argument."""
    env = os.environ.get("EPL_LMHEAD_LIVE_ROWS")
    if env == "0":
        return False
    if env == "1":
        return True
    return bool(flag)


def pad_rows(count):
    return (count + PAD_ROWS - 1) // PAD_ROWS * PAD_ROWS


def _native_ok(t):
    return (t.dim() == 2 and t.is_contiguous()
            and t.dtype in (torch.bfloat16, torch.float32)
            and 1 <= t.shape[0] < 2 ** 31 and t.shape[1] >= 1
            and (t.shape[1] * t.element_size()) % 16 == 0
            and t.data_ptr() % 16 == 0)


def live_rows_mode(g2, x2, weight):
    """"native" (HIP kernels), "torch" (CPU boolean indexing) or None
    (dense) for a backward with these operands."""
    if g2.shape[0] == 0 or not (g2.dtype == x2.dtype == weight.dtype):
        return None
    if not g2.is_cuda:
        return "torch"
    if torch.cuda.is_current_stream_capturing():
        return None     # the host read of count cannot be captured
    if not (use_native(g2) and _native_ok(g2) and _native_ok(x2)):
        return None
    return "native"


# ---- the three operations, twice ---------------------------------------------
def rows_live_index(g2, mode):
    """-> (idx, count, inv); count is a 1-element tensor (native) or an int
    (torch).  torch: idx is the int64 list of live rows, inv the bool mask."""
    if mode == "native":
        return native_ext().rows_live_index(g2)
    live = (g2 != 0).any(dim=1)
    idx = live.nonzero().squeeze(1)
    return idx, int(idx.numel()), live


def gather_rows(src, idx, count, n_pad, mode):
    if mode == "native":
        return native_ext().gather_rows(src, idx, count, n_pad)
    out = src.new_zeros((n_pad, src.shape[1]))
    out[:count] = src[idx]
    return out


def scatter_rows_zero(src, idx, count, inv, rows, mode):
    if mode == "native":
        return native_ext().scatter_rows_zero(src, inv)
    out = src.new_zeros((rows, src.shape[1]))
    out[inv] = src[:count]
    return out


# ---- the two backward paths ---------------------------------------------------
def dense_backward(g2, x2, weight):
    """(dX [N, H], dW [V, H]): the GEMMs autograd issues for F.linear."""
    return g2 @ weight, g2.t() @ x2


def live_rows_backward(g2, x2, weight, mode):
    """(dX, dW) from the live rows of g2, or None when half the rows or
    more are live (the caller then runs dense_backward)."""
    rows = g2.shape[0]
    idx, count, inv = rows_live_index(g2, mode)
    n_live = int(count)         # native: the backward's one host sync
    if n_live == 0:
        return torch.zeros_like(x2), torch.zeros_like(weight)
    n_pad = pad_rows(n_live)
    if n_pad >= DENSE_FRACTION * rows:
        return None
    g_c = gather_rows(g2, idx, count, n_pad, mode)
    x_c = gather_rows(x2, idx, count, n_pad, mode)
    dw = g_c.t() @ x_c
    dx_c = g_c @ weight
    return scatter_rows_zero(dx_c, idx, count, inv, rows, mode), dw


class LiveRowsLinear(torch.autograd.Function):
    """``F.linear(x, weight)`` (no bias) with the backward above."""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return F.linear(x, weight)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        g2 = dy.reshape(-1, dy.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        mode = live_rows_mode(g2, x2, weight)
        out = None
        if mode is not None:
            out = live_rows_backward(g2, x2, weight, mode)
        if out is None:
            out = dense_backward(g2, x2, weight)
        dx, dw = out
        return dx.view(x.shape), dw
