"""Bias + GeLU forward / backward and the column-sum kernel pair
(csrc/kernels/kernels.hip) against the fp64 references of kernel_refs.py,
with the derived per-element bounds.

Direct _C.bias_gelu_fwd / _C.bias_gelu_bwd / _C.colsum calls on inputs
from a seeded CPU generator: randn plus a sweep of x + bias over every
bf16 value of [-12, 12] and +-40, dy with one sign down a column and dy
that cancels down a column.  Every case asserts

* |got - ref| <= 2 E on the bf16 tensors and <= E on dbias, the fp32
  column sums and the fp32 tensors (the fp32 path's E carries the
  cancellation of its 1 - 2 / (e^2u + 1) form as an absolute term);
* every result is finite;
* every sentinel in the guard rows around out and dx, around dbias, db
  and the column sum's partial workspace is untouched.

Each case prints its worst err / E per output (``GELU-RATIO`` and
``COLSUM-RATIO`` lines; the table in docs/testing.md is made from them).
"""

import pytest
import torch

from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _collect(bufs, stray):
    torch.cuda.synchronize()
    for key, buf in bufs.items():
        n = buf.stray_writes()
        if n:
            stray.append("%d stray writes around %s" % (n, key))
    return {key: buf.view.cpu().to(F64) for key, buf in bufs.items()}


@pytest.mark.parametrize("rows,cols,bf16", kr.gelu_cases())
def test_bias_gelu_fp64(rows, cols, bf16):
    from easyparallellibrary_amd import _C
    dtype = torch.bfloat16 if bf16 else torch.float32
    stray = []

    def run(inp):
        x, bias, dy = (inp[k].to(dtype).cuda() for k in ("x", "bias", "dy"))
        bufs = {"out": kr.guarded_rows(rows, cols, dtype, "cuda"),
                "dx": kr.guarded_rows(rows, cols, dtype, "cuda"),
                "dbias": kr.attn_flat(cols, torch.float32, "cuda")}
        bufs["dbias"].view.zero_()        # the kernels accumulate into it
        _C.bias_gelu_fwd(bufs["out"].view, x, bias)
        _C.bias_gelu_bwd(bufs["dx"].view, bufs["dbias"].view, dy, x, bias)
        got = _collect(bufs, stray)
        for key, t in got.items():
            if not bool(torch.isfinite(t).all()):
                stray.append(key + " not finite")
        return got

    worst, bad = kr.gelu_check_case(
        rows, cols, bf16, run,
        kr.GELU_FACTOR_BF16 if bf16 else kr.GELU_FACTOR_F32)
    print("GELU-RATIO rows %d cols %d bf16 %d %s"
          % (rows, cols, bf16, kr.format_worst(worst)))
    assert not bad and not stray, (bad, stray)


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("rows", kr.COLSUM_ROWS)
@pytest.mark.parametrize("cols", kr.COLSUM_COLS)
def test_colsum_fp64(cols, rows, bf16):
    """fused_colsum's kernel pair at its own stripe count: 1 stripe at
    rows 1 and 5, 1024 stripes of 5 rows at 4099 (the last 204 stripes own
    no row and must write zeros, the one before them owns 4)"""
    from easyparallellibrary_amd import _C
    from easyparallellibrary_amd.ops.bias_linear import _stripes_for
    dtype = torch.bfloat16 if bf16 else torch.float32
    stripes = _stripes_for(rows, cols)
    assert stripes == (1 if rows < 8 else 1024)
    worst, bad = {}, []
    for name in kr.LN_DY_FAMILIES:
        gen = torch.Generator().manual_seed(rows + cols)
        dy = kr.dy_family(name, rows, cols, gen)
        bufs = {"db": kr.attn_flat(cols, dtype, "cuda"),
                "partial": kr.attn_flat(stripes * cols, torch.float32,
                                        "cuda")}
        _C.colsum(dy.to(dtype).cuda(), bufs["db"].view, bufs["partial"].view)
        got = _collect(bufs, bad)
        r = kr.ratio_of(got["db"], kr.colsum_ref(dy),
                        kr.colsum_bounds(dy, bf16))
        worst[name] = r
        if not r <= (2.0 if bf16 else 1.0):
            bad.append("%s err/E %.3g" % (name, r))
        if not bool(torch.isfinite(got["partial"]).all()):
            bad.append("partial workspace not fully written")
    print("COLSUM-RATIO cols %d rows %d bf16 %d %s" % (
        cols, rows, bf16, " ".join("%s=%.3f" % kv for kv in worst.items())))
    assert not bad, bad
