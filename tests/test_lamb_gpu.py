"""lamb_phase1 / lamb_phase2 called directly, and FusedLAMB.step, against
the fp64 reference of tests/kernel_refs.py.

The arena is built by production code (FlatParamGroup + FusedLAMB) over
bf16 parameters of shapes (3,), (130,), (64, 33), (1,), (257,), (4000,):
padded extents 128 ... 4096, a separate fp32 master.  Chunk c's weights
and gradients are scaled by 10**(c % 4), so eight elements counted into a
neighbouring chunk move that chunk's norm by far more than any tolerance.
One parameter is all zero (||w|| = 0) and, at weight_decay 0, one has a
zero gradient at step 1 (||u|| = 0): both must take trust ratio 1.

In the direct phase tests, hyper-parameters that the kernels take as fp32
(betas, lr) are given as fp32-representable doubles to kernel and
reference alike, so the comparison is of the same operation on the same
inputs: 1 - fp32(0.999) differs from 0.001 by 1.3e-5 relative, more than
the tolerance on v.  The FusedLAMB.step tests give the reference the
optimizer's own doubles, which the kernel rounds to fp32; that difference
(at most 1.3e-5 relative) disappears inside their 1e-3 bound.
"""

import pytest
import torch

from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from easyparallellibrary_amd import _C
else:
    _C = None

F64 = torch.float64


def dev():
    return torch.device("cuda:0")


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


B1, B2, EPS, LR = f32(0.9), f32(0.999), 1e-6, f32(1e-2)


def _group(grad_dtype, shapes=kr.LAMB_SHAPES, zero_param=1, **opt_kw):
    from easyparallellibrary_amd.parallel.dp import FlatParamGroup
    from easyparallellibrary_amd.runtime.optim import FusedLAMB
    params = kr.lamb_params(shapes, torch.bfloat16, dev(), zero_param)
    g = FlatParamGroup(params, dev())
    opt = FusedLAMB([g], **opt_kw)
    if grad_dtype != g.grad_arena.dtype:
        # a bf16 parameter cannot own an fp32 .grad; the kernel's fp32-grad
        # branch gets a flat fp32 arena of the same layout instead
        g.grad_arena = torch.zeros(g.total, dtype=grad_dtype, device=dev())
    kr.lamb_fill(g, seed=1, grad_mul=0.0, scale_weights=True)
    # what the kernels index with, against the buffers they index
    kr.check_chunk_map(g)
    n = g.total
    assert g.master_arena.dtype == torch.float32
    assert g.master_arena is not g.param_arena
    for t in (g.master_arena, g.param_arena, g.grad_arena,
              g.state["exp_avg"], g.state["exp_avg_sq"],
              g.state["lamb_update"]):
        assert t.numel() == n and t.is_contiguous()
    assert g.state["lamb_chunk_of"].numel() * 8 == n
    return g, opt


def _cpu64(t):
    return t.detach().cpu().to(F64)


def _ulp32(x):
    """fp32 unit in the last place at |x| (fp64 tensor), 0 at 0."""
    ax = x.abs()
    e = torch.floor(torch.log2(torch.where(ax > 0, ax, torch.ones_like(ax))))
    return torch.where(ax > 0, 2.0 ** (e - 23), torch.zeros_like(ax))


@pytest.mark.parametrize("inv_scale", [1.0, 1.0 / 1024])
@pytest.mark.parametrize("wd", [0.01, 0.0])
@pytest.mark.parametrize("grad_dtype", [torch.bfloat16, torch.float32])
def test_lamb_phase1(grad_dtype, wd, inv_scale):
    """m, v, update: atol 1e-6 * the chunk's magnitude, rtol 1e-5 (the
    fused_adamw tolerances).  wsq / usq are fp32 atomic sums of n_c
    non-negative terms in arbitrary order, worst case n_c * 2**-24
    relative; each chunk is held to twice that, (n_c + 2) * 2**-23 with
    n_c the padded extent (<= 4096, so < 1e-3), against the fp64 sum of
    the very terms the kernel summed (master, and its own update output,
    which is checked element by element first).  usq is also compared with
    the reference's own ||u||^2, with the elementwise tolerance on u
    carried through the square added to the bound."""
    g, _ = _group(grad_dtype)
    ext = kr.lamb_extents(g)
    pext = kr.lamb_padded_extents(g)
    pad = kr.lamb_padding_mask(g)
    mag = kr.lamb_elem_magnitude(g)
    nch = len(ext)
    master64 = _cpu64(g.master_arena)
    zero_chunk = [c for c, (o, n) in enumerate(ext)
                  if not master64[o:o + n].any()]
    assert len(zero_chunk) == 1
    m64 = torch.zeros_like(master64)
    v64 = torch.zeros_like(master64)
    m, v, upd = (g.state["exp_avg"], g.state["exp_avg_sq"],
                 g.state["lamb_update"])
    for step in (1, 2, 3):
        kr.lamb_fill(g, seed=20 + step, grad_mul=1.0 / inv_scale,
                     zero_grad_chunk=1 if step == 1 else None)
        ref = kr.lamb_ref(master64, _cpu64(g.grad_arena), m64, v64, ext, LR,
                          B1, B2, EPS, wd, step, inv_scale)
        wsq = torch.zeros(nch, dtype=torch.float32, device=dev())
        usq = torch.zeros(nch, dtype=torch.float32, device=dev())
        upd.fill_(float("nan"))
        _C.lamb_phase1(g.master_arena, g.grad_arena, m, v, upd,
                       g.state["lamb_chunk_of"], wsq, usq, B1, B2, EPS, wd,
                       step, inv_scale)
        torch.cuda.synchronize()
        assert torch.equal(_cpu64(g.master_arena), master64)
        tol_u = None
        for name, got, want in (("m", m, ref["m"]), ("v", v, ref["v"]),
                                ("update", upd, ref["update"])):
            got = _cpu64(got)
            tol = 1e-6 * mag + 1e-5 * want.abs()
            err = (got - want).abs()
            print("step %d %s: max err/tol %.3g" %
                  (step, name, (err / tol).max().item()))
            assert torch.isfinite(got).all(), name
            assert (err <= tol).all(), (step, name, (err / tol).max())
            assert (got[pad] == 0).all(), name
            tol_u = tol
        u_got = _cpu64(upd)
        wsq, usq = _cpu64(wsq), _cpu64(usq)
        for c, ((off, n), (_, n_c)) in enumerate(zip(ext, pext)):
            rtol_c = (n_c + 2) * 2.0 ** -23
            w_terms = (master64[off:off + n] ** 2).sum()
            u_terms = (u_got[off:off + n] ** 2).sum()
            assert abs(wsq[c] - w_terms) <= rtol_c * w_terms, (step, c)
            assert abs(usq[c] - u_terms) <= rtol_c * u_terms, (step, c)
            ur = ref["update"][off:off + n]
            tu = tol_u[off:off + n]
            slack = (2 * ur.abs() * tu + tu * tu).sum()
            assert abs(usq[c] - ref["usq"][c]) <= \
                rtol_c * ref["usq"][c] + slack, (step, c)
            assert abs(wsq[c] - ref["wsq"][c]) <= rtol_c * ref["wsq"][c]
        rel_w = ((wsq - ref["wsq"]).abs() / ref["wsq"].clamp_min(1e-300))
        print("step %d: max rel err wsq %.3g" % (step, rel_w.max().item()))
        assert wsq[zero_chunk[0]] == 0
        if wd == 0.0 and step == 1:
            assert usq[1] == 0 and ref["usq"][1] == 0
        m64, v64 = ref["m"], ref["v"]


@pytest.mark.parametrize("with_bf16", [True, False])
def test_lamb_phase2(with_bf16):
    """master - lr * ratio[c] * update with chosen ratios (0.5 + c), within
    2 fp32 ulps of |master| of the fp64 expression.  The update is built as
    +/- |master| * U(0.5, 4), so lr * ratio * update is at most 0.22 |master|
    and the two roundings of the product plus the one of the difference
    stay under 2**-23 |master| <= 2 ulps; an fma changes that by less.
    The all-zero parameter has no |master| to measure against: there the
    bound is 2 ulps of the expected value."""
    g, _ = _group(torch.bfloat16)
    pad = kr.lamb_padding_mask(g)
    pext = kr.lamb_padded_extents(g)
    master64 = _cpu64(g.master_arena)
    gen = torch.Generator().manual_seed(5)
    u = (torch.rand(g.total, generator=gen) * 3.5 + 0.5) * \
        torch.where(torch.rand(g.total, generator=gen) < 0.5, -1.0, 1.0)
    u = u * torch.where(master64 != 0, master64.abs(),
                        torch.ones_like(master64)).float()
    u[pad] = 0
    ratio = torch.arange(len(pext), dtype=torch.float32) + 0.5
    per_elem = torch.zeros(g.total, dtype=F64)
    for c, (off, n_c) in enumerate(pext):
        per_elem[off:off + n_c] = ratio[c].item()
    want = master64 - LR * per_elem * u.to(F64)
    param_before = g.param_arena.clone()
    g.state["lamb_update"].copy_(u)
    _C.lamb_phase2(g.master_arena, g.param_arena if with_bf16 else None,
                   g.state["lamb_update"], g.state["lamb_chunk_of"],
                   ratio.to(dev()), LR)
    torch.cuda.synchronize()
    got = _cpu64(g.master_arena)
    bound = 2 * _ulp32(torch.where(master64 != 0, master64, want))
    err = (got - want).abs()
    live = bound > 0
    print("phase2: max err / ulp(|master|) %.3g" %
          (2 * err[live] / bound[live]).max().item())
    assert (err <= bound).all()
    assert (got != master64)[~pad].all()      # every element moved
    assert (got[pad] == 0).all()
    if with_bf16:
        assert torch.equal(g.param_arena,
                           g.master_arena.to(torch.bfloat16))
        assert (g.param_arena[pad.to(dev())] == 0).all()
    else:
        assert torch.equal(g.param_arena, param_before)


def _check_steps(g, opt, steps, grad_scale, zero_grad_chunk):
    """|d_got - d_ref| <= 1e-3 |d_ref| + 2**-22 |master| for each step's
    change d of the master: the (n_c + 2) * 2**-23 < 1e-3 bound on each
    norm carried through sqrt(wsq / usq) (which halves it), plus the
    elementwise 1e-5 on u, plus 2 ulps of the master for the update
    arithmetic."""
    ext = kr.lamb_extents(g)
    pad = kr.lamb_padding_mask(g)
    m64 = torch.zeros(g.total, dtype=F64)
    v64 = torch.zeros(g.total, dtype=F64)
    for step in range(1, steps + 1):
        kr.lamb_fill(g, seed=40 + step, grad_mul=grad_scale,
                     zero_grad_chunk=zero_grad_chunk if step == 1 else None)
        before = _cpu64(g.master_arena)
        ref = kr.lamb_ref(before, _cpu64(g.grad_arena), m64, v64, ext,
                          opt.lr, opt.beta1, opt.beta2, opt.eps,
                          opt.weight_decay, step, 1.0 / grad_scale)
        opt.step(grad_scale=grad_scale)
        torch.cuda.synchronize()
        after = _cpu64(g.master_arena)
        d_got, d_ref = after - before, ref["master"] - before
        tol = 1e-3 * d_ref.abs() + 2.0 ** -22 * before.abs()
        err = (d_got - d_ref).abs()
        print("step %d: max err/tol %.3g, max |d_got-d_ref|/|d_ref| %.3g" %
              (step, (err / tol.clamp_min(1e-300)).max().item(),
               (err / d_ref.abs().clamp_min(1e-30))[~pad].max().item()))
        assert torch.isfinite(after).all()
        assert (err <= tol).all(), (step, (err / tol.clamp_min(1e-300)).max())
        assert (after[pad] == 0).all()
        assert torch.equal(g.param_arena, g.master_arena.to(torch.bfloat16))
        m64, v64 = ref["m"], ref["v"]
    assert opt.step_count == steps


def test_lamb_step_matches_fp64():
    import easyparallellibrary_amd as epl
    epl.init()
    g, opt = _group(torch.bfloat16, lr=1e-2, weight_decay=0.01)
    _check_steps(g, opt, 3, 1024.0, zero_grad_chunk=1)


def test_lamb_step_zero_norms_take_ratio_one():
    """weight_decay 0: the zero-gradient chunk (||u|| = 0) must not move
    at step 1, and the all-zero chunk (||w|| = 0) moves by lr * u."""
    import easyparallellibrary_amd as epl
    epl.init()
    g, opt = _group(torch.float32, lr=1e-2, weight_decay=0.0)
    _check_steps(g, opt, 2, 1.0, zero_grad_chunk=1)


def test_lamb_grid_stride():
    """300 parameters of 4000 elements: 300 * 4096 = 1,228,800 arena
    elements, more than the 4096 * 256 threads of one grid pass; every
    chunk is 4096 elements, so the bound of _check_steps still applies."""
    import easyparallellibrary_amd as epl
    epl.init()
    g, opt = _group(torch.bfloat16, shapes=[(4000,)] * 300, zero_param=None,
                    lr=1e-2, weight_decay=0.01)
    assert g.total == 300 * 4096 > 4096 * 256
    _check_steps(g, opt, 1, 1.0, zero_grad_chunk=None)
