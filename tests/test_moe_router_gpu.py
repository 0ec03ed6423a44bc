"""The fused MoE router kernels (csrc/kernels/moe_router.hip) called
directly through _C, against the fp64 reference and the derived
per-element bounds of tests/moe_router_refs.py (proven on the CPU by
test_moe_router_refs_cpu.py on the same cases).

Shapes: N in {1, 63, 64, 65, 1000} x E in {2, 8, 24, 64, 100, 256} x k in
{1, 2} x {bf16, fp32}: E = 8 / 24 / 64 / 256 take the vector loads of the
1 / 4 / 8 / 64 lane groupings, E = 2 and 100 the element-wise ones (rows
not 16-byte aligned), with -inf padding inside the group at 2, 24 and
100; one E = 8 case runs from buffers that are not 16-byte aligned; one
has more tokens than a grid pass holds.  Families: see
moe_router_refs.router_logits.

Every output starts as NaN (the int64 ones as a sentinel) inside a guarded
buffer.  topi and counts equal the reference exactly, fp32 outputs are
within 1.0 x E, bf16 dlogits within 2.0 x E, guards are intact and two
runs are bitwise equal.
"""

import pytest
import torch

from tests import kernel_refs as kr
from tests import moe_router_refs as rr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from easyparallellibrary_amd import _C
else:
    _C = None

F64 = torch.float64
GUARD = 64
INT_SENTINEL = -0x5A5A5A5A5A5A5A5B
DTYPE_IDS = {torch.bfloat16: "bf16", torch.float32: "fp32"}
E_DTYPE = [(e, dt) for e in rr.ROUTER_E for dt in rr.ROUTER_DTYPES]
E_DTYPE_IDS = ["E{}-{}".format(e, DTYPE_IDS[dt]) for e, dt in E_DTYPE]


def dev():
    return torch.device("cuda:0")


class _IntBuffer:
    """a guarded int64 buffer (kernel_refs.GuardedBuffer holds 2- and
    4-byte types)"""

    def __init__(self, n):
        self.raw = torch.full((n + 2 * GUARD,), INT_SENTINEL,
                              dtype=torch.long, device=dev())
        self.view = self.raw[GUARD:GUARD + n]
        self.n = n

    def stray_writes(self):
        raw = self.raw.cpu()
        return int((raw[:GUARD] != INT_SENTINEL).sum() +
                   (raw[GUARD + self.n:] != INT_SENTINEL).sum())


def _run_once(z, k, dw, dtype, misalign=0):
    """forward, then backward on the forward's own lse / topi / counts;
    returns the outputs (device) and the buffers"""
    n, e = z.shape
    d = dev()
    guard = GUARD + misalign
    zbuf = kr.GuardedBuffer((n, e), (e, 1), 0, dtype, d, guard)
    zbuf.view.copy_(z.to(dtype))
    bufs = dict(
        topi=_IntBuffer(n * k), counts=_IntBuffer(e),
        topw=kr.attn_flat(n * k, torch.float32, d),
        lse=kr.attn_flat(n, torch.float32, d),
        psum=kr.attn_flat(e, torch.float32, d),
        losses=kr.attn_flat(2, torch.float32, d),
        dz=kr.GuardedBuffer((n, e), (e, 1), 0, dtype, d, guard))
    v = {key: b.view for key, b in bufs.items()}
    _C.moe_router_fwd(zbuf.view, k, v["topi"], v["topw"], v["lse"],
                      v["counts"], v["psum"], v["losses"])
    g_bal = torch.tensor(rr.G_BAL, dtype=torch.float32, device=d)
    g_z = torch.tensor(rr.G_Z, dtype=torch.float32, device=d)
    _C.moe_router_bwd(v["dz"], zbuf.view, v["lse"], v["topi"],
                      dw.to(torch.float32).to(d).contiguous(), v["counts"],
                      g_bal, g_z, k)
    torch.cuda.synchronize()
    bufs["z"] = zbuf
    return v, bufs


def _check(family, n, e, k, dtype, worst, misalign=0):
    z = rr.router_logits(family, n, e, dtype)
    dw = rr.router_dw(n, k)
    ref = rr.router_ref(z, k, dw, rr.G_BAL, rr.G_Z)
    bounds = rr.router_bounds(ref, z, k, dtype)
    v, bufs = _run_once(z, k, dw, dtype, misalign)
    v2, _ = _run_once(z, k, dw, dtype, misalign)
    tag = (family, n, e, k, DTYPE_IDS[dtype])
    for key in v:
        a, b = v[key], v2[key]
        if a.dtype == torch.bfloat16:
            a, b = a.view(torch.int16), b.view(torch.int16)
        elif a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), (tag, key, "run to run")
    for key, b in bufs.items():
        assert b.stray_writes() == 0, (tag, key)
    assert torch.equal(bufs["z"].view.cpu().to(F64), z), tag
    losses = v["losses"].cpu().to(F64)
    got = dict(topi=v["topi"].cpu().reshape(n, k), counts=v["counts"].cpu(),
               topw=v["topw"].cpu().reshape(n, k), lse=v["lse"].cpu(),
               psum=v["psum"].cpu(), l_bal=losses[0], l_z=losses[1],
               dz=v["dz"].cpu())
    for key in ("topw", "lse", "psum", "dz"):
        assert not torch.isnan(got[key].float()).any(), (tag, key)
    assert not torch.isnan(losses).any(), tag
    assert int(got["counts"].sum()) == n * k
    if family == "equal" and k == 2:
        assert bool((got["topi"] == torch.tensor([0, 1])).all()), tag
    ratios = rr.router_ratios(got, ref, bounds)
    allowed = rr.router_allowed(dtype)
    for key, r in ratios.items():
        worst[key] = max(worst.get(key, 0.0), r)
    bad = ["{} err/E {:.3f} > {}".format(key, r, allowed[key])
           for key, r in ratios.items() if not r <= allowed[key]]
    return ["{}: {}".format(tag, b) for b in bad]


def _report(label, worst):
    print("%s worst err / E: %s" % (
        label, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("e,dtype", E_DTYPE, ids=E_DTYPE_IDS)
def test_router_kernels(e, dtype):
    worst, bad = {}, []
    for n, k, family in rr.router_cases(e):
        bad += _check(family, n, e, k, dtype, worst)
    _report("E %d %s" % (e, DTYPE_IDS[dtype]), worst)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", rr.ROUTER_DTYPES,
                         ids=[DTYPE_IDS[d] for d in rr.ROUTER_DTYPES])
def test_router_unaligned_buffers(dtype):
    """E = 8 from logits / dlogits that start 2 (bf16) or 4 (fp32) bytes
    past a 16-byte boundary: the element-wise path"""
    worst, bad = {}, []
    for k in rr.ROUTER_K:
        bad += _check("ties", 65, 8, k, dtype, worst, misalign=1)
    _report("unaligned E 8 %s" % DTYPE_IDS[dtype], worst)
    assert not bad, "\n".join(bad)


def test_router_grid_stride():
    n, e = rr.ROUTER_GRID_STRIDE
    # tokens one pass of the largest grid holds at one lane per token
    assert n > _C.moe_router_waves(n, e) * 64
    worst = {}
    bad = _check("randn", n, e, 2, torch.bfloat16, worst)
    _report("grid stride N %d E %d bf16" % (n, e), worst)
    assert not bad, "\n".join(bad)
