"""LayerNorm forward and backward (csrc/kernels/kernels.hip) against the
fp64 references of kernel_refs.py, with the derived per-element bounds.

Direct _C.layer_norm_fwd / _C.layer_norm_bwd_fused calls on inputs built
by a seeded CPU generator: rows of the families randn / offset /
near_const / const / tiny / one_hot in turn, with and without a residual,
gamma and beta with a zero and a negative column, dy with one sign down a
column and dy that cancels down a column.  The backward runs on the
forward's own s, mean and rstd, as the module does.  Every case asserts

* |got - ref| <= 2 E on the bf16 tensors (out, s, dx) and <= E on mean,
  rstd, dgamma, dbeta, colsum and the fp32 tensors (kernel_refs derives
  the E's; test_kernel_refs_cpu.py proves them for the rounding model and
  shows that they reject twelve wrong kernels);
* every result is finite;
* every sentinel in the two guard rows before and after out, s and dx and
  in the guards around mean, rstd, dgamma, dbeta and colsum is untouched.

Each case prints its worst err / E per output and family (``LN-RATIO``
lines; the table in docs/testing.md is made from them).
"""

import pytest
import torch

from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

F64 = torch.float64


class Kernels:
    """the two callbacks of kr.ln_check_case on the GPU; collects the
    stray writes of every launch"""

    def __init__(self, bf16):
        from easyparallellibrary_amd import _C
        self.c = _C
        self.dtype = torch.bfloat16 if bf16 else torch.float32
        self.stray = []

    def dev(self, t):
        return None if t is None else t.to(self.dtype).cuda().contiguous()

    def collect(self, label, bufs):
        torch.cuda.synchronize()
        for key, buf in bufs.items():
            n = buf.stray_writes()
            if n:
                self.stray.append("%s: %d stray writes around %s"
                                  % (label, n, key))
        return {key: buf.view.cpu().to(F64) for key, buf in bufs.items()}

    def fwd(self, inp, with_res):
        rows, cols = inp["x"].shape
        bufs = {"out": kr.guarded_rows(rows, cols, self.dtype, "cuda"),
                "mean": kr.attn_flat(rows, torch.float32, "cuda"),
                "rstd": kr.attn_flat(rows, torch.float32, "cuda")}
        if with_res:
            bufs["s"] = kr.guarded_rows(rows, cols, self.dtype, "cuda")
        self.c.layer_norm_fwd(
            bufs["out"].view, self.dev(inp["x"]), self.dev(inp["res"]),
            bufs["s"].view if with_res else None, self.dev(inp["gamma"]),
            self.dev(inp["beta"]), bufs["mean"].view, bufs["rstd"].view,
            kr.LN_EPS)
        return self.collect("fwd res%d" % with_res, bufs)

    def bwd(self, inp, x_used, mean, rstd, dadd, want_colsum):
        rows, cols = x_used.shape
        bufs = {"dx": kr.guarded_rows(rows, cols, self.dtype, "cuda"),
                "dgamma": kr.attn_flat(cols, torch.float32, "cuda"),
                "dbeta": kr.attn_flat(cols, torch.float32, "cuda")}
        if want_colsum:
            bufs["colsum"] = kr.attn_flat(cols, torch.float32, "cuda")
        for key in ("dgamma", "dbeta", "colsum"):
            if key in bufs:          # the kernels accumulate into these
                bufs[key].view.zero_()
        self.c.layer_norm_bwd_fused(
            bufs["dx"].view, bufs["dgamma"].view, bufs["dbeta"].view,
            self.dev(inp["dy"]), self.dev(x_used), self.dev(inp["gamma"]),
            mean.float().cuda(), rstd.float().cuda(), self.dev(dadd),
            bufs["colsum"].view if want_colsum else None)
        return self.collect("bwd dadd%d cs%d" % (dadd is not None,
                                                 want_colsum), bufs)


@pytest.mark.parametrize("cols,rows,bf16", kr.ln_cases())
def test_layer_norm_fp64(cols, rows, bf16):
    k = Kernels(bf16)
    worst, bad = kr.ln_check_case(
        cols, rows, bf16, k.fwd, k.bwd,
        kr.LN_FACTOR_BF16 if bf16 else kr.LN_FACTOR_F32)
    print("LN-RATIO cols %d rows %d bf16 %d %s"
          % (cols, rows, bf16, kr.format_worst(worst)))
    assert not bad and not k.stray, (bad[:8], len(bad), k.stray[:8])
