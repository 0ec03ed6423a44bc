"""The flat-arena utility kernels called directly: sqnorm against the fp64
sum within sqnorm_bounds (tests/optim_refs.py), scale_ / f32_to_bf16 /
bf16_to_f32 exact against torch's own casts on edge bit patterns, and the
refusals of the bindings (no launch happens there)."""

import numpy as np
import pytest
import torch

from tests import kernel_refs as kr
from tests import optim_refs as orf
from tests.optim_refs import BF16, F32

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from easyparallellibrary_amd import _C
else:
    _C = None

GUARD = 64
SQNORM_NS = (0, 1, 255, 257, 777, 1024 * 256, 1024 * 256 + 77)
PAST_GRID = orf.GRID_PASS + 13


def dev():
    return torch.device("cuda:0")


def _guarded(values, n=None):
    n = values.numel() if n is None else n
    b = kr.attn_flat(n, values.dtype, dev(), GUARD)
    b.view[:values.numel()].copy_(values)
    return b


def _sqnorm(x, out0=0.0):
    """x (CPU) through the kernel from a guarded buffer into a guarded
    one-element accumulator holding out0"""
    src = _guarded(x)
    out = _guarded(torch.tensor([out0], dtype=F32))
    before = src.raw.clone()
    _C.sqnorm(src.view, out.view)
    torch.cuda.synchronize()
    assert src.stray_writes() == 0 and out.stray_writes() == 0
    assert torch.equal(src.raw, before)
    return float(out.view.cpu()[0])


def _sqnorm_data(kind, n, dtype, gen):
    if kind == "randn":
        x = torch.randn(n, generator=gen)
    elif kind == "spike":       # one 2^40 among 2^-20
        x = torch.full((n,), 2.0 ** -20)
        if n:
            x[n // 2] = 2.0 ** 40
    else:
        x = torch.full((n,), 1.5)
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("n", SQNORM_NS)
def test_sqnorm_within_bounds(n, dtype):
    gen = torch.Generator().manual_seed(n)
    for kind in ("randn", "spike", "equal"):
        for out0 in (0.0, 3.25):
            x = _sqnorm_data(kind, n, dtype, gen)
            ref = orf.sqnorm_ref(x, out0)
            e = orf.sqnorm_bounds(n, ref)
            got = _sqnorm(x, out0)
            err = abs(got - ref)
            print("sqnorm n %d %s out0 %g: err/E %.3g" %
                  (n, kind, out0, err / e if err else 0.0))
            assert err <= e, (kind, out0, got, ref)
            if n == 0:
                assert got == out0


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_sqnorm_non_finite(dtype):
    n = 1024 * 256 + 77
    base = torch.ones(n).to(dtype)
    for at in (0, 255, 256, n // 2, n - 1):
        for bad in (float("inf"), float("-inf"), float("nan")):
            x = base.clone()
            x[at] = bad
            got = _sqnorm(x)
            assert not np.isfinite(got), (at, bad, got)
    # finite data whose sum is past the fp32 maximum: +Inf, never NaN
    x = torch.full((777,), 2.0 ** 63).to(dtype)
    assert orf.sqnorm_ref(x) > 3.5e38 and float(x.float().pow(2).max()) < 1e38
    assert _sqnorm(x) == float("inf")


def _cast_values(n):
    """fp32 test vector of n elements: the edge patterns first, randn
    behind them; the patterns again at the very end (the tail)"""
    edge = orf.f32_from_bits(orf.cast_edge_values())
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    k = min(n, edge.numel())
    x[:k] = edge[:k]
    if n >= 2 * edge.numel():
        x[-edge.numel():] = edge
    return x


def _bits_equal(a, b):
    return orf.same_bits(a.cpu(), b.cpu())


def _nan_aware_equal(a, b):
    """same bits, except that any NaN matches any NaN"""
    a, b = a.cpu(), b.cpu()
    an, bn = torch.isnan(a.float()), torch.isnan(b.float())
    return torch.equal(an, bn) and orf.same_bits(
        torch.where(an, torch.zeros_like(a), a),
        torch.where(bn, torch.zeros_like(b), b))


@pytest.mark.parametrize("n", [1, 7, 8, 1001, PAST_GRID])
def test_f32_to_bf16_exact(n):
    x = _cast_values(n)
    src, dst = _guarded(x), kr.attn_flat(n, BF16, dev(), GUARD)
    _C.f32_to_bf16(dst.view, src.view)
    torch.cuda.synchronize()
    assert src.stray_writes() == 0 and dst.stray_writes() == 0
    want = x.to(BF16)
    assert _nan_aware_equal(dst.view, want)
    assert _bits_equal(src.view, x)


def test_f32_to_bf16_all_high_halves():
    """every high half under the low halves that decide the rounding"""
    bits = orf.all_bit_patterns()
    x = orf.f32_from_bits(bits)
    src, dst = _guarded(x), kr.attn_flat(x.numel(), BF16, dev(), GUARD)
    _C.f32_to_bf16(dst.view, src.view)
    torch.cuda.synchronize()
    assert dst.stray_writes() == 0
    assert _nan_aware_equal(dst.view, x.to(BF16))
    # bit for bit the rounding add on everything that is not a NaN
    got = orf.bf16_bits(dst.view)
    nan = (bits & 0x7fffffff) > 0x7f800000
    assert np.array_equal(got[~nan], orf.f2bf_parent(bits)[~nan])
    assert bool(((got[nan] & 0x7fff) > 0x7f80).all())


@pytest.mark.parametrize("n", [1, 7, 8, 1001, PAST_GRID])
def test_bf16_to_f32_exact(n):
    x = _cast_values(n).to(BF16)
    src, dst = _guarded(x), kr.attn_flat(n, F32, dev(), GUARD)
    _C.bf16_to_f32(dst.view, src.view)
    torch.cuda.synchronize()
    assert src.stray_writes() == 0 and dst.stray_writes() == 0
    assert _nan_aware_equal(dst.view, x.float())


def test_bf16_to_f32_all_patterns():
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)
    src, dst = _guarded(pats), kr.attn_flat(65536, F32, dev(), GUARD)
    _C.bf16_to_f32(dst.view, src.view)
    torch.cuda.synchronize()
    assert dst.stray_writes() == 0
    assert _nan_aware_equal(dst.view, pats.float())
    # a widening keeps even a NaN's payload
    assert _bits_equal(dst.view, pats.float())


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("n", [1, 7, 8, 1001, PAST_GRID])
def test_scale_exact(n, dtype):
    """x * s rounded once: torch's own fp32 product, cast back to bf16 by
    torch.  s = 0.5 keeps every bit pattern but the smallest denormals;
    s = 0.3 rounds everywhere."""
    for s in (0.5, orf.f32(0.3)):
        x = _cast_values(n).to(dtype)
        buf = _guarded(x)
        _C.scale_(buf.view, s)
        torch.cuda.synchronize()
        assert buf.stray_writes() == 0
        want = (x.float() * torch.tensor(s, dtype=F32)).to(dtype)
        assert _nan_aware_equal(buf.view, want), s


# ---------------------------------------------------------------------------
# refusals: every one of these raises before any launch
# ---------------------------------------------------------------------------
def _adamw_args(n=1024, gdt=BF16, with_param=True):
    d = dev()
    return dict(master=torch.zeros(n, device=d),
                param=torch.zeros(n, device=d, dtype=BF16) if with_param
                else None,
                grad=torch.zeros(n, device=d, dtype=gdt),
                m=torch.zeros(n, device=d), v=torch.zeros(n, device=d))


def _adamw(a):
    _C.fused_adamw(a["master"], a["param"], a["grad"], a["m"], a["v"], 1e-3,
                   0.9, 0.999, 1e-8, 0.01, 1, 1.0)


def test_fused_adamw_accepts_what_production_passes():
    for gdt in (BF16, F32):
        a = _adamw_args(1024, gdt)
        _adamw({k: (t[128:640] if t is not None else None)
                for k, t in a.items()})
        _adamw(dict(a, param=None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["master", "param", "grad", "m", "v"])
def test_fused_adamw_refuses(name):
    for gdt in (BF16, F32):
        good = _adamw_args(1024, gdt)
        wide = _adamw_args(2048, gdt)
        cases = {
            "cpu": good[name].cpu(),
            "non-contiguous": wide[name][::2],
            "size": wide[name][:1016],
            "dtype": good[name].to(torch.float16),
            # one element off the base: 4 bytes of fp32, 2 of bf16
            "alignment": wide[name][1:1025],
        }
        if name == "grad":      # either of the two gradient dtypes is fine
            cases["dtype"] = good[name].to(torch.float64)
        for what, t in cases.items():
            assert t.numel() == 1024 or what == "size"
            with pytest.raises(RuntimeError):
                _adamw(dict(good, **{name: t}))
        # aligned for 16 bytes only: enough for bf16, not for fp32
        t = wide[name][4:1028] if wide[name].dtype == F32 else None
        if t is not None:
            with pytest.raises(RuntimeError):
                _adamw(dict(good, **{name: t}))
        for k in ("master", "m", "v"):      # nothing ran
            assert not good[k].any()


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_sqnorm_and_scale_refuse(dtype):
    d = dev()
    x = torch.ones(2048, device=d, dtype=dtype)
    out = torch.zeros(1, device=d)
    for bad in (x.cpu(), x[::2], x.to(torch.float16)):
        with pytest.raises(RuntimeError):
            _C.sqnorm(bad, out)
        with pytest.raises(RuntimeError):
            _C.scale_(bad, 0.5)
    for bad_out in (out.cpu(), out.double(), torch.zeros(4, device=d)[::2]):
        with pytest.raises(RuntimeError):
            _C.sqnorm(x, bad_out)
    with pytest.raises(RuntimeError):
        _C.scale_(x[1:1025], 0.5)           # 2 or 4 bytes off the base
    torch.cuda.synchronize()
    assert float(out) == 0.0 and bool((x == 1).all())
    # sqnorm has element loads: any element offset is fine
    _C.sqnorm(x[1:1025], out)
    torch.cuda.synchronize()
    assert float(out) == 1024.0
