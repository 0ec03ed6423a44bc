"""The fp64 router reference, its bounds and its emulation
(tests/moe_router_refs.py), proven without a GPU on the cases the GPU test
(test_moe_router_gpu.py) runs."""

import pytest
import torch

from easyparallellibrary_amd.ops import moe
from tests import moe_router_refs as rr

F64 = torch.float64
DTYPE_IDS = {torch.bfloat16: "bf16", torch.float32: "fp32"}
E_DTYPE = [(e, dt) for e in rr.ROUTER_E for dt in rr.ROUTER_DTYPES]
E_DTYPE_IDS = ["E{}-{}".format(e, DTYPE_IDS[dt]) for e, dt in E_DTYPE]


def _case(family, n, e, k, dtype):
    z = rr.router_logits(family, n, e, dtype)
    dw = rr.router_dw(n, k)
    ref = rr.router_ref(z, k, dw, rr.G_BAL, rr.G_Z)
    return z, dw, ref


def _autograd(z, k, dw, g_bal, g_z):
    """the plain formulas under torch fp64 autograd"""
    n, e = z.shape
    zz = z.clone().requires_grad_(True)
    lse = torch.logsumexp(zz, dim=1)
    p = torch.softmax(zz, dim=1)
    topi = torch.sort(z, dim=1, descending=True,
                      stable=True).indices[:, :k]
    psel = p.gather(1, topi)
    w = psel / psel.sum(dim=1, keepdim=True)
    counts = torch.bincount(topi.reshape(-1), minlength=e)
    f = counts.to(F64) / (n * k)
    l_bal = e * (f * p.mean(dim=0)).sum()
    l_z = (lse ** 2).mean()
    ((dw * w).sum() + g_bal * l_bal + g_z * l_z).backward()
    return dict(lse=lse.detach(), topw=w.detach(), l_bal=l_bal.detach(),
                l_z=l_z.detach(), psum=p.detach().sum(dim=0), dz=zz.grad,
                topi=topi, counts=counts)


@pytest.mark.parametrize("e,dtype", E_DTYPE, ids=E_DTYPE_IDS)
def test_reference_matches_fp64_autograd(e, dtype):
    for n, k, family in rr.router_cases(e):
        z, dw, ref = _case(family, n, e, k, dtype)
        auto = _autograd(z, k, dw, rr.G_BAL, rr.G_Z)
        assert torch.equal(auto["topi"], ref["topi"])
        assert torch.equal(auto["counts"], ref["counts"])
        for key in ("lse", "topw", "l_bal", "l_z", "psum", "dz"):
            err = (auto[key] - ref[key]).abs()
            tol = 1e-12 * (1 + ref[key].abs())
            if key == "dz" and k == 2:
                # the weights' term divides by S: 1e-12 of its magnitude
                tol = tol + 1e-12 * (dw.abs().sum(dim=1) /
                                     ref["ssel"])[:, None]
            assert bool((err <= tol).all()), (family, n, k, key,
                                              float((err / tol).max()))


@pytest.mark.parametrize("e,dtype", E_DTYPE, ids=E_DTYPE_IDS)
def test_emulation_within_bounds(e, dtype):
    worst = {}
    for n, k, family in rr.router_cases(e):
        z, dw, ref = _case(family, n, e, k, dtype)
        bounds = rr.router_bounds(ref, z, k, dtype)
        emu = rr.router_emulate(z, k, dw, rr.G_BAL, rr.G_Z, dtype)
        ratios = rr.router_ratios(emu, ref, bounds)
        for key, r in ratios.items():
            assert r <= (0.0 if key in ("topi", "counts") else 1.0), \
                (family, n, k, key, r)
            worst[key] = max(worst.get(key, 0.0), r)
    print("E %d %s emulation worst err / E: %s" % (
        e, DTYPE_IDS[dtype],
        ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def test_emulation_grid_stride_case():
    n, e = rr.ROUTER_GRID_STRIDE
    z, dw, ref = _case("randn", n, e, 2, torch.bfloat16)
    bounds = rr.router_bounds(ref, z, 2, torch.bfloat16)
    emu = rr.router_emulate(z, 2, dw, rr.G_BAL, rr.G_Z, torch.bfloat16)
    for key, r in rr.router_ratios(emu, ref, bounds).items():
        assert r <= (0.0 if key in ("topi", "counts") else 1.0), (key, r)


@pytest.mark.parametrize("e,dtype", [(2, torch.float32),
                                     (8, torch.bfloat16),
                                     (24, torch.float32),
                                     (100, torch.bfloat16)])
def test_torch_path_matches_reference(e, dtype):
    """ops.moe.router_torch, the module's torch path, forward and (by
    autograd) backward, held to the kernels' bounds: autograd, too, rounds
    the gradient once to the logits' dtype"""
    for n, k, family in rr.router_cases(e):
        z, dw, ref = _case(family, n, e, k, dtype)
        bounds = rr.router_bounds(ref, z, k, dtype)
        logits = z.to(dtype).requires_grad_(True)
        topi, topw, counts, l_bal, l_z = moe.router_torch(logits, k)
        ((dw.float() * topw).sum() + rr.G_BAL * l_bal +
         rr.G_Z * l_z).backward()
        assert topw.dtype == torch.float32 and counts.dtype == torch.long
        got = dict(topi=topi, counts=counts, topw=topw.detach(),
                   l_bal=l_bal.detach(), l_z=l_z.detach(), dz=logits.grad)
        for key, r in rr.router_ratios(got, ref, bounds).items():
            assert r <= (0.0 if key in ("topi", "counts") else 1.0), \
                (family, n, k, key, r)


@pytest.mark.parametrize("e", rr.ROUTER_E)
def test_families_have_their_properties(e):
    n = rr.ROUTER_ALL_FAMILIES_N
    for dtype in rr.ROUTER_DTYPES:
        props = {fam: {k: rr.router_properties(
            rr.router_logits(fam, n, e, dtype), k) for k in rr.ROUTER_K}
            for fam in rr.ROUTER_FAMILIES}
        assert props["ties"][2]["tie12"]
        assert props["ties"][2]["tie23"] == (e >= 3)
        assert props["equal"][2]["tie12"]
        assert props["spread90"][1]["underflow"]
        for k in rr.ROUTER_K:
            assert props["never"][k]["empty_expert"] == (e > k)
        assert props["randn"][1]["top3_distinct"] or \
            dtype == torch.bfloat16
    # an all-equal row selects experts 0 and 1
    z = rr.router_logits("equal", 5, e, torch.bfloat16)
    ref = rr.router_ref(z, 2)
    assert torch.equal(ref["topi"], torch.tensor([[0, 1]] * 5))
    # ties go to the lower index
    z = rr.router_logits("ties", 64, e, torch.bfloat16)
    ref = rr.router_ref(z, 2)
    v = z.gather(1, ref["topi"])
    assert bool(((v[:, 0] > v[:, 1]) |
                 (ref["topi"][:, 0] < ref["topi"][:, 1])).all())


# (mutation, family, N, E, k): where the wrong kernel has to show
MUTATION_CASES = {
    "tie_high": ("ties", 64, 8, 2),
    "f_after_capacity": ("equal", 1000, 8, 2),
    "lse_nomax": ("shift1000", 64, 8, 2),
    "no_pa": ("randn", 65, 24, 2),
    "lse1": ("randn", 63, 64, 1),
}


@pytest.mark.parametrize("mutation", rr.MUTATIONS)
def test_mutations_are_caught(mutation):
    """five wrong kernels, as mutations of the reference, each exceed the
    allowed bound at least tenfold somewhere (the threshold of
    test_kernel_refs_cpu.py)"""
    family, n, e, k = MUTATION_CASES[mutation]
    for dtype in rr.ROUTER_DTYPES:
        z, dw, ref = _case(family, n, e, k, dtype)
        bounds = rr.router_bounds(ref, z, k, dtype)
        bad = rr.router_ref(z, k, dw, rr.G_BAL, rr.G_Z, mutate=mutation)
        bad["dz"] = rr.round_to(bad["dz"], dtype)
        ratios = rr.router_ratios(bad, ref, bounds)
        allowed = rr.router_allowed(dtype)
        worst = max((r / allowed[key] if allowed[key] > 0 else
                     (float("inf") if r > 0 else 0.0))
                    for key, r in ratios.items())
        assert worst >= 10.0, (mutation, dtype, ratios)
        # and the unmutated reference, rounded the same way, passes
        good = dict(ref)
        good["dz"] = rr.round_to(ref["dz"], dtype)
        for key, r in rr.router_ratios(good, ref, bounds).items():
            assert r <= allowed[key], (key, r)
