"""llama_refs.py validated without a GPU:

* the references equal torch fp64 autograd of the plain formulas (HF
  rotate_half, F.silu, the hand-written RMSNorm) to 1e-12;
* the fp32 emulations, which round where the kernels round, stay within
  the criterion on every case of the GPU matrices;
* the rotation is orthogonal (inverse after forward is the identity);
* every wrong kernel of a list, written as a mutation of a reference,
  exceeds the allowed error at least tenfold on some element.
"""

import pytest
import torch
import torch.nn.functional as F

from tests import kernel_refs as kr
from tests import llama_refs as lr

F64 = torch.float64


def _close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale


# ---- references against autograd ------------------------------------------
def _rotate_half(x):
    half = x.shape[-1] // 2
    return torch.cat([-x[..., half:], x[..., :half]], dim=-1)


@pytest.mark.parametrize("d", lr.ROPE_DIMS)
def test_rope_ref_is_hf_rotate_half(d):
    seq, pos0 = 33, 17
    cos, sin = lr.rope_tables_ref(d, lr.ROPE_THETA, 64)
    x = lr.rope_input(seq, d, 3).requires_grad_()
    c = torch.cat([cos, cos], -1)[pos0:pos0 + seq].to(F64)[None, :, None, :]
    s = torch.cat([sin, sin], -1)[pos0:pos0 + seq].to(F64)[None, :, None, :]
    y_hf = x * c + _rotate_half(x) * s
    y, _ = lr.rope_ref(x.detach(), cos, sin, pos0)
    _close(y, y_hf.detach())
    g = torch.randn(y.shape, dtype=F64,
                    generator=torch.Generator().manual_seed(1))
    y_hf.backward(g)
    # the backward of the rotation is the inverse rotation of the gradient
    gx, _ = lr.rope_ref(g, cos, sin, pos0, inverse=True)
    _close(gx, x.grad)


def test_rope_tables_of_the_op_are_the_reference_tables():
    from easyparallellibrary_amd.ops.rope import rope_tables
    for d in lr.ROPE_DIMS:
        cos, sin = rope_tables("cpu", d, lr.ROPE_THETA, 4000 + 257)
        assert cos.dtype == torch.float32 and cos.shape == (8192, d // 2)
        rc, rs = lr.rope_tables_ref(d, lr.ROPE_THETA, 8192)
        assert torch.equal(cos, rc) and torch.equal(sin, rs)


@pytest.mark.parametrize("d,seq,pos0", lr.rope_cases())
def test_rope_orthogonal_and_emulation_within_bound(d, seq, pos0):
    cos, sin = lr.rope_tables_ref(d, lr.ROPE_THETA, 8192)
    x = lr.rope_input(seq, d, 2 * lr.ROPE_H)
    for inverse in (False, True):
        y, m = lr.rope_ref(x, cos, sin, pos0, inverse)
        back, _ = lr.rope_ref(y, cos, sin, pos0, not inverse)
        # cos^2 + sin^2 of the fp32 tables is 1 to 2^-23
        assert float((back - x).abs().max()) <= 2.0 ** -21 * float(
            x.abs().max())
        r = lr.ratio_of(lr.rope_emulate(x, cos, sin, pos0, inverse), y,
                        lr.rope_bounds(y, m))
        assert r <= lr.FACTOR["y"], r


def test_rms_ref_is_autograd():
    rows, cols = 5, 40
    inp = lr.ln_inputs(rows, cols, True)
    x, res, gamma = (inp[k].clone().requires_grad_()
                     for k in ("x", "res", "gamma"))
    s = x + res
    s.retain_grad()
    rstd = (s.pow(2).mean(dim=1, keepdim=True) + lr.RMS_EPS).rsqrt()
    out = s * rstd * gamma
    ref = lr.rms_ref(inp["x"], inp["res"], inp["gamma"])
    _close(ref["out"], out.detach())
    _close(ref["rstd"], rstd.detach().squeeze(1))
    dy, dadd = inp["dy"], inp["dadd"]
    # dadd arrives through the summed stream
    (out * dy).sum().add((s * dadd).sum()).backward()
    b = lr.rms_bwd_ref(dy, ref["s"], inp["gamma"], ref["rstd"], dadd)
    _close(b["dx"], x.grad)
    _close(b["dx"], res.grad)
    _close(b["dgamma"], gamma.grad)


def test_swiglu_ref_is_autograd():
    inp = lr.swiglu_inputs(3, 520)
    gu = inp["gu"].clone().requires_grad_()
    f = gu.shape[1] // 2
    out = F.silu(gu[:, :f]) * gu[:, f:]
    out.backward(inp["dy"])
    ref = lr.swiglu_ref(inp["gu"], inp["dy"])
    _close(ref["out"], out.detach())
    _close(torch.cat([ref["dgate"], ref["dup"]], dim=1), gu.grad)


# ---- emulations within the criterion on the GPU matrices ------------------
def _rms_emulated(cols, rows):
    def fwd(inp, with_res):
        return lr.rms_emulate(inp["x"], inp["res"], inp["gamma"])

    def bwd(inp, dy, s_used, rstd, dadd):
        return lr.rms_bwd_emulate(dy, s_used, inp["gamma"], rstd, dadd)

    return lr.rms_check_case(cols, rows, fwd, bwd)


@pytest.mark.parametrize("cols,rows", lr.rms_cases())
def test_rms_emulation_within_bound(cols, rows):
    worst, bad = _rms_emulated(cols, rows)
    assert not bad, bad


def test_rms_paths_cover_every_instantiation():
    fwd = {(lr.rms_fwd_path(c)["chunks"], lr.rms_fwd_path(c)["block"])
           for c in lr.RMS_COLS}
    assert {c for c, _ in fwd} == {1, 2, 4}
    assert {b for _, b in fwd} == {64, 128, 192, 256}
    bwd = {(lr.rms_bwd_path(c)["block"], lr.rms_bwd_path(c)["chunks"])
           for c in lr.RMS_COLS}
    assert bwd == {(False, 1), (False, 2), (False, 4), (True, 2), (True, 4)}
    # both sides of the wave / block boundary
    assert not lr.rms_bwd_path(2048)["block"] and lr.rms_bwd_path(2056)["block"]
    # the grid-stride cases own more rows than the launch has teams
    for cols, rows in lr.RMS_GRID_CASES:
        assert rows > 4096 >= lr.rms_bwd_parts(rows, cols)


@pytest.mark.parametrize("rows,f", lr.swiglu_cases())
def test_swiglu_emulation_within_bound(rows, f):
    worst, bad = lr.swiglu_check_case(
        rows, f, lambda inp: lr.swiglu_emulate(inp["gu"], inp["dy"]))
    assert not bad, bad


def test_swiglu_matrix_properties():
    sweep = lr.swiglu_sweep()
    for e in lr.SWIGLU_EXTREMES:
        assert bool((sweep == e).any()) and bool((sweep == -e).any())
    assert bool((lr.bf16_round(sweep) == sweep).all())
    # the whole sweep is present once the shape has room for it
    assert lr.swiglu_inputs(37, 512)["nsweep"] == sweep.numel()
    # one case needs more than one pass at the launcher's cap
    assert lr.swiglu_passes(1025, 4096) == 2
    assert max(lr.swiglu_passes(r, f) for r, f in lr.swiglu_cases()) >= 2
    # g = -100: the reference and the emulation give a finite zero
    gu = torch.tensor([[-100.0] * 8 + [1.5] * 8], dtype=F64)
    dy = torch.ones(1, 8, dtype=F64)
    em = lr.swiglu_emulate(gu, dy)
    assert all(bool(torch.isfinite(t).all()) for t in em.values())
    assert float(em["out"].abs().max()) == 0.0


# ---- mutations: every wrong kernel is far outside --------------------------
def _worst(got, want, bound):
    return lr.ratio_of(got, want, bound)


ROPE_MUTATIONS = ("interleaved", "pos_off_by_one", "pos0_ignored",
                  "inverse_for_forward", "v_rotated", "half_unrotated")


@pytest.mark.parametrize("name", ROPE_MUTATIONS)
def test_rope_mutation_caught(name):
    d, seq, pos0, h = 64, 33, 4000, lr.ROPE_H
    cos, sin = lr.rope_tables_ref(d, lr.ROPE_THETA, 8192)
    # the packed buffer [B, S, 3, H, D]: q and k rotate, v keeps its bits
    packed = lr.rope_input(seq, d, 3 * h).reshape(lr.ROPE_B, seq, 3, h, d)
    qk = packed[:, :, :2].reshape(lr.ROPE_B, seq, 2 * h, d)
    y, m = lr.rope_ref(qk, cos, sin, pos0)
    want = torch.cat([y.reshape(lr.ROPE_B, seq, 2, h, d), packed[:, :, 2:]],
                     dim=2)
    bound = torch.cat([lr.rope_bounds(y, m).reshape(lr.ROPE_B, seq, 2, h, d),
                       torch.zeros_like(packed[:, :, 2:])], dim=2)
    c = cos[pos0:pos0 + seq].to(F64)[None, :, None, :]
    s = sin[pos0:pos0 + seq].to(F64)[None, :, None, :]
    if name == "interleaved":
        x1, x2 = qk[..., 0::2], qk[..., 1::2]
        got = torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
        got = got.reshape(qk.shape)
    elif name == "pos_off_by_one":
        got, _ = lr.rope_ref(qk, cos, sin, pos0 + 1)
    elif name == "pos0_ignored":
        got, _ = lr.rope_ref(qk, cos, sin, 0)
    elif name == "inverse_for_forward":
        got, _ = lr.rope_ref(qk, cos, sin, pos0, inverse=True)
    elif name == "half_unrotated":
        got = torch.cat([y[..., :d // 2], qk[..., d // 2:]], dim=-1)
    else:
        got = y
    got = torch.cat([got.reshape(lr.ROPE_B, seq, 2, h, d), packed[:, :, 2:]],
                    dim=2)
    if name == "v_rotated":
        allr, _ = lr.rope_ref(packed.reshape(lr.ROPE_B, seq, 3 * h, d), cos,
                              sin, pos0)
        got = allr.reshape(packed.shape)
    assert _worst(lr.bf16_round(got), want, bound) >= 10 * lr.FACTOR["y"]


RMS_MUTATIONS = ("mean_subtracted", "eps_dropped", "last_vector_unsummed",
                 "residual_after_statistic", "dx_without_projection",
                 "dadd_dropped", "dgamma_misses_last_row", "gamma_shifted")


@pytest.mark.parametrize("name", RMS_MUTATIONS)
def test_rms_mutation_caught(name):
    rows, cols = 37, 520
    inp = lr.ln_inputs(rows, cols, True)
    x, res, gamma = inp["x"], inp["res"], inp["gamma"]
    ref = lr.rms_ref(x, res, gamma)
    e = lr.rms_fwd_bounds(ref, x, res, gamma)
    s, eps = ref["s"], lr.RMS_EPS
    dy, dadd = inp["dy"], inp["dadd"]
    bref = lr.rms_bwd_ref(dy, s, gamma, ref["rstd"], dadd)
    eb = lr.rms_bwd_bounds(bref, dy, s, gamma, ref["rstd"], dadd)
    if name == "mean_subtracted":
        dev = s - s.mean(dim=1, keepdim=True)
        got = dev * ((dev * dev).mean(dim=1, keepdim=True) + eps) ** -0.5 \
            * gamma
        r = _worst(lr.bf16_round(got), ref["out"], e["out"])
    elif name == "eps_dropped":
        got = ref["ms"] ** -0.5       # inf on the all-zero row
        r = _worst(got, ref["rstd"], e["rstd"])
    elif name == "last_vector_unsummed":
        got = ((s[:, :-8] ** 2).sum(dim=1) / cols + eps) ** -0.5
        r = _worst(got, ref["rstd"], e["rstd"])
    elif name == "residual_after_statistic":
        got = s * ((x * x).mean(dim=1, keepdim=True) + eps) ** -0.5 * gamma
        r = _worst(lr.bf16_round(got), ref["out"], e["out"])
    elif name == "gamma_shifted":
        got = s * ref["rstd"][:, None] * torch.roll(gamma, 8)
        r = _worst(lr.bf16_round(got), ref["out"], e["out"])
    elif name == "dx_without_projection":
        got = bref["dyg"] * ref["rstd"][:, None] + dadd
        r = _worst(lr.bf16_round(got), bref["dx"], eb["dx"])
    elif name == "dadd_dropped":
        r = _worst(lr.bf16_round(bref["o"]), bref["dx"], eb["dx"])
    else:
        got = (dy[:-1] * bref["xhat"][:-1]).sum(dim=0)
        r = _worst(got, bref["dgamma"], eb["dgamma"])
    fp32 = name in ("eps_dropped", "last_vector_unsummed",
                    "dgamma_misses_last_row")
    assert r >= 10 * (1.0 if fp32 else 2.0), r


SWIGLU_MUTATIONS = ("gate_up_exchanged", "gelu_for_silu",
                    "derivative_without_gs1s", "dup_into_gate_half")


@pytest.mark.parametrize("name", SWIGLU_MUTATIONS)
def test_swiglu_mutation_caught(name):
    inp = lr.swiglu_inputs(37, 520)
    gu, dy = inp["gu"], inp["dy"]
    ref = lr.swiglu_ref(gu, dy)
    e = lr.swiglu_bounds(ref, dy)
    g, up, s = ref["g"], ref["up"], ref["s"]
    if name == "gate_up_exchanged":
        got, key = up * torch.sigmoid(up) * g, "out"
    elif name == "gelu_for_silu":
        got, key = kr.gelu_tanh(g) * up, "out"
    elif name == "derivative_without_gs1s":
        got, key = dy * up * s, "dgate"
    else:
        got, key = ref["dup"], "dgate"
    r = _worst(lr.bf16_round(got), ref[key], e[key])
    assert r >= 10 * lr.FACTOR[key], r
