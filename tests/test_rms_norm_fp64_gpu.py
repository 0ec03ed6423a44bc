"""RMSNorm forward / backward (csrc/kernels/llama_ops.hip) against the
fp64 references of llama_refs.py, with the derived per-element bounds.

Direct _C.rms_norm_fwd / _C.rms_norm_bwd calls on inputs from a seeded CPU
generator: the LayerNorm row kinds (randn, offsets, near-constant rows, an
all-zero row whose rstd is eps^-1/2, tiny rows, one-hot rows) in every
rotation, with and without the fused residual add; the backward at the
kernel's own s and rstd, with and without dadd, for dy with one sign down a
column and dy that cancels down a column.  Widths cover every CHUNKS of
both kernels, the wave / block boundary of the backward (2048 | 2056) and
the grid-stride loops (4099 x 64, 8191 x 512).  Every case asserts

* |got - ref| <= 2 E on out, s, dx (bf16) and <= E on rstd, dgamma (fp32);
* every result is finite;
* every sentinel in the guard rows around the outputs is untouched;
* a second run of the same launch gives the same bits.

Each case prints its worst err / E per output (``RMS-RATIO`` lines; the
table in docs/testing.md is made from them).
"""

import pytest
import torch

from tests import kernel_refs as kr
from tests import llama_refs as lr

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16


@pytest.mark.parametrize("cols,rows", lr.rms_cases())
def test_rms_norm_fp64(cols, rows):
    from easyparallellibrary_amd import _C
    trouble = []

    def launch_twice(make_bufs, launch):
        """run ``launch(bufs)`` on two fresh sets of guarded buffers and
        compare every bit, guards included"""
        first = make_bufs()
        launch(first)
        second = make_bufs()
        launch(second)
        torch.cuda.synchronize()
        for key in first:
            if not torch.equal(first[key].raw, second[key].raw):
                trouble.append("two runs differ in " + key)
            n = first[key].stray_writes()
            if n:
                trouble.append("%d stray writes around %s" % (n, key))
        return {key: buf.view.cpu().to(F64) for key, buf in first.items()}

    def fwd(inp, with_res):
        x = inp["x"].to(BF16).cuda()
        res = inp["res"].to(BF16).cuda() if with_res else None
        gamma = inp["gamma"].to(BF16).cuda()

        def make():
            bufs = {"out": kr.guarded_rows(rows, cols, BF16, "cuda"),
                    "rstd": kr.attn_flat(rows, torch.float32, "cuda")}
            if with_res:
                bufs["s"] = kr.guarded_rows(rows, cols, BF16, "cuda")
            return bufs

        def launch(bufs):
            _C.rms_norm_fwd(bufs["out"].view, x, res,
                            bufs["s"].view if with_res else None, gamma,
                            bufs["rstd"].view, lr.RMS_EPS)

        return launch_twice(make, launch)

    def bwd(inp, dy, s_used, rstd, dadd):
        dy_d = dy.to(BF16).cuda()
        s_d = s_used.to(BF16).cuda()
        gamma = inp["gamma"].to(BF16).cuda()
        rstd_d = rstd.float().cuda()
        dadd_d = dadd.to(BF16).cuda() if dadd is not None else None

        def make():
            return {"dx": kr.guarded_rows(rows, cols, BF16, "cuda"),
                    "dgamma": kr.attn_flat(cols, torch.float32, "cuda")}

        def launch(bufs):
            _C.rms_norm_bwd(bufs["dx"].view, bufs["dgamma"].view, dy_d, s_d,
                            gamma, rstd_d, dadd_d)

        return launch_twice(make, launch)

    worst, bad = lr.rms_check_case(cols, rows, fwd, bwd)
    print("RMS-RATIO cols %d rows %d %s" % (cols, rows,
                                            kr.format_worst(worst)))
    assert not bad and not trouble, (bad, trouble)


def test_rms_norm_const0_row_is_exact():
    """the all-zero row: rstd = eps^-1/2 and out = 0, whatever gamma"""
    from easyparallellibrary_amd import _C
    cols = 512
    x = torch.zeros(3, cols, dtype=BF16, device="cuda")
    gamma = torch.randn(cols).to(BF16).cuda()
    out = torch.full_like(x, float("nan"))
    rstd = torch.full((3,), float("nan"), device="cuda")
    _C.rms_norm_fwd(out, x, None, None, gamma, rstd, lr.RMS_EPS)
    assert float(out.float().abs().max()) == 0.0
    want = lr.RMS_EPS ** -0.5
    assert float((rstd.double() - want).abs().max()) <= 2.0 ** -22 * want


@pytest.mark.parametrize("dtype,cols", [(torch.float32, 1000), (BF16, 8200),
                                        (BF16, 1004)])
def test_rms_norm_refused_width_runs_through_torch(dtype, cols):
    """a dtype or width the native path does not take (fp32, past 8192, no
    multiple of 8): the binding refuses it, the module computes it in
    torch"""
    from easyparallellibrary_amd import _C
    from easyparallellibrary_amd.ops.rms_norm import FusedRMSNorm
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(5, cols, generator=gen).to(dtype).cuda()
    res = torch.randn(5, cols, generator=gen).to(dtype).cuda()
    gamma = torch.randn(cols, generator=gen).to(dtype).cuda()
    out, s = torch.empty_like(x), torch.empty_like(x)
    rstd = torch.empty(5, device="cuda")
    with pytest.raises(RuntimeError):
        _C.rms_norm_fwd(out, x, res, s, gamma, rstd, lr.RMS_EPS)
    with pytest.raises(RuntimeError):
        _C.rms_norm_bwd(out, torch.empty(cols, device="cuda"), x, s, gamma,
                        rstd, None)
    mod = FusedRMSNorm(cols).to("cuda", dtype)
    with torch.no_grad():
        mod.weight.copy_(gamma)
    xr = x.clone().requires_grad_()
    y, ssum = mod.forward_with_sum(xr, res)
    (y.float().sum() + ssum.float().sum()).backward()
    ref = lr.rms_ref(x.cpu().to(F64), res.cpu().to(F64), gamma.cpu().to(F64))
    tol = 2.0 ** -7 if dtype == BF16 else 1e-5
    err = (y.detach().cpu().to(F64) - ref["out"]).abs()
    assert bool((err <= tol * (1 + ref["out"].abs())).all())
    assert bool(torch.isfinite(xr.grad).all())
    assert bool(torch.isfinite(mod.weight.grad).all())
