"""The fixed-order, typed column reductions behind layer_norm_bwd_typed and
bias_gelu_bwd_typed (partial_rows_reduce_kernel, csrc/kernels/kernels.hip).

The LN and bias-GeLU backward kernels leave one fp32 partial row per block
(per wave segment) and one reduce kernel sums them in a fixed order, one
writer per column, and stores the sum in the dtype of the tensor it is
handed.  Checked here, against the fp64 references of kernel_refs.py:

* outputs handed in FULL OF NaN, as bf16 and as fp32, come back finite and
  within the bound: nothing has to be zeroed first;
* the bound is the derived fp32 bound E32 of ln_bwd_bounds /
  bias_gelu_bounds, plus one bf16 rounding V |ref| (V = kr.V_BF16 = 2^-9)
  for a bf16 output.  It is applied as every bf16 tensor of this suite is
  (test_layer_norm_fp64_gpu.py, the bf16 colsum): at 2 E, because round to
  nearest of an 8-bit significand errs by up to 2^-8 relative just above a
  power of two; fp32 outputs at 1 E (measured on an MI355X: bf16 outputs
  up to 1.99 E, all of it the final rounding, fp32 outputs up to 0.61 E);
* two calls give torch.equal results (no float atomics);
* the older bindings, called with zeroed fp32 outputs as the existing
  tests call them, still meet the same fp32 bounds, twice in a row with
  equal bits.

LN shapes: cols 256 / 1000 / 1024 / 2048 x rows 1 / 3 / 5 / 4100.
Bias-GeLU: cols 512 / 4096 x rows 1 / 7 / 3000.
"""

import pytest
import torch

from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF = torch.bfloat16
LN_COLS = (256, 1000, 1024, 2048)
LN_ROWS = (1, 3, 5, 4100)
GELU_COLS = (512, 4096)
GELU_ROWS = (1, 7, 3000)


def nan_out(n, dtype):
    """guarded [n] output, every addressed element NaN"""
    buf = kr.attn_flat(n, dtype, "cuda")
    buf.view.fill_(float("nan"))
    return buf


def check(bad, label, got, ref, e32, dtype):
    got = got.cpu()
    if not bool(torch.isfinite(got).all()):
        bad.append(label + " not finite")
        return 0.0
    if dtype == BF:
        e, factor = e32 + kr.V_BF16 * ref.abs(), 2.0
    else:
        e, factor = e32, 1.0
    r = kr.ratio_of(got.to(F64), ref, e)
    if not r <= factor:
        bad.append("%s err/E %.3g > %g" % (label, r, factor))
    return r


@pytest.mark.parametrize("cols", LN_COLS)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_ln_typed_reduce(rows, cols):
    from easyparallellibrary_amd import _C
    inp = kr.ln_inputs(rows, cols, False,
                       dy_name="cancel" if rows == 3 else "coherent")
    x, gamma, dy, dadd = inp["x"], inp["gamma"], inp["dy"], inp["dadd"]
    fwd = kr.ln_ref(x, None, gamma, inp["beta"])
    mean, rstd = kr.f32_round(fwd["mean"]), kr.f32_round(fwd["rstd"])
    ref = kr.ln_bwd_ref(dy, x, gamma, mean, rstd, dadd)
    e = kr.ln_bwd_bounds(ref, dy, x, gamma, mean, rstd, dadd, True)
    dev = dict(dy=dy.to(BF).cuda(), x=x.to(BF).cuda(),
               gamma=gamma.to(BF).cuda(), mean=mean.float().cuda(),
               rstd=rstd.float().cuda(), dadd=dadd.to(BF).cuda())
    keys = ("dgamma", "dbeta", "colsum")
    bad, worst = [], {}

    def typed(dtype):
        dx = kr.guarded_rows(rows, cols, BF, "cuda")
        outs = {k: nan_out(cols, dtype) for k in keys}
        _C.layer_norm_bwd_typed(
            dx.view, outs["dgamma"].view, outs["dbeta"].view, dev["dy"],
            dev["x"], dev["gamma"], dev["mean"], dev["rstd"], dev["dadd"],
            outs["colsum"].view)
        torch.cuda.synchronize()
        for k, b in list(outs.items()) + [("dx", dx)]:
            if b.stray_writes():
                bad.append("%s: stray writes around %s" % (dtype, k))
        return dict({k: b.view.clone() for k, b in outs.items()},
                    dx=dx.view.clone())

    for dtype in (BF, torch.float32):
        first, second = typed(dtype), typed(dtype)
        for k in keys:
            worst["%s/%s" % (k, "bf16" if dtype == BF else "f32")] = check(
                bad, "typed %s %s" % (dtype, k), first[k], ref[k], e[k],
                dtype)
        for k in first:
            if not torch.equal(first[k], second[k]):
                bad.append("typed %s %s: two calls differ" % (dtype, k))

    def old():
        dx = torch.empty(rows, cols, dtype=BF, device="cuda")
        outs = {k: torch.zeros(cols, dtype=torch.float32, device="cuda")
                for k in keys}
        _C.layer_norm_bwd_fused(dx, outs["dgamma"], outs["dbeta"],
                                dev["dy"], dev["x"], dev["gamma"],
                                dev["mean"], dev["rstd"], dev["dadd"],
                                outs["colsum"])
        return dict(outs, dx=dx)

    first, second = old(), old()
    for k in keys:
        worst[k + "/old"] = check(bad, "old binding " + k, first[k], ref[k],
                                  e[k], torch.float32)
    for k in first:
        if not torch.equal(first[k], second[k]):
            bad.append("old binding %s: two calls differ" % k)
    print("LNTYPED-RATIO cols %d rows %d %s" % (cols, rows, " ".join(
        "%s=%.3f" % kv for kv in sorted(worst.items()))))
    assert not bad, (bad[:8], len(bad))


@pytest.mark.parametrize("cols", GELU_COLS)
@pytest.mark.parametrize("rows", GELU_ROWS)
def test_bias_gelu_typed_reduce(rows, cols):
    from easyparallellibrary_amd import _C
    bad, worst = [], {}
    # both dy families on the small shapes; the tall one keeps its fp64
    # reference to one (coherent at 512 columns, cancel at 4096)
    names = kr.LN_DY_FAMILIES if rows < 1000 else (
        kr.LN_DY_FAMILIES[0 if cols == 512 else 1],)
    for dy_name in names:
        inp = kr.bias_gelu_inputs(rows, cols, dy_name)
        ref = kr.bias_gelu_ref(inp["x"], inp["bias"], inp["dy"])
        e = kr.bias_gelu_bounds(ref, inp["x"], inp["bias"], inp["dy"], True)
        dev = {k: inp[k].to(BF).cuda() for k in ("x", "bias", "dy")}

        def typed(dtype):
            dx = kr.guarded_rows(rows, cols, BF, "cuda")
            db = nan_out(cols, dtype)
            _C.bias_gelu_bwd_typed(dx.view, db.view, dev["dy"], dev["x"],
                                   dev["bias"])
            torch.cuda.synchronize()
            if dx.stray_writes() or db.stray_writes():
                bad.append("%s %s: stray writes" % (dy_name, dtype))
            return dx.view.clone(), db.view.clone()

        for dtype in (BF, torch.float32):
            (dx1, db1), (dx2, db2) = typed(dtype), typed(dtype)
            tag = "%s/%s" % (dy_name, "bf16" if dtype == BF else "f32")
            worst[tag] = check(bad, "typed dbias " + tag, db1, ref["dbias"],
                               e["dbias"], dtype)
            r = kr.ratio_of(dx1.cpu().to(F64), ref["dx"], e["dx"])
            if not r <= kr.GELU_FACTOR_BF16["dx"]:
                bad.append("typed dx %s err/E %.3g" % (tag, r))
            if not (torch.equal(dx1, dx2) and torch.equal(db1, db2)):
                bad.append("typed %s: two calls differ" % tag)

        def old():
            dx = torch.empty(rows, cols, dtype=BF, device="cuda")
            db = torch.zeros(cols, dtype=torch.float32, device="cuda")
            _C.bias_gelu_bwd(dx, db, dev["dy"], dev["x"], dev["bias"])
            return dx, db

        (dx1, db1), (dx2, db2) = old(), old()
        worst[dy_name + "/old"] = check(bad, "old binding dbias " + dy_name,
                                        db1, ref["dbias"], e["dbias"],
                                        torch.float32)
        if not (torch.equal(dx1, dx2) and torch.equal(db1, db2)):
            bad.append("old binding %s: two calls differ" % dy_name)
    print("GELUTYPED-RATIO cols %d rows %d %s" % (cols, rows, " ".join(
        "%s=%.3f" % kv for kv in sorted(worst.items()))))
    assert not bad, (bad[:8], len(bad))
