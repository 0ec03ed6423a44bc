"""The AdamW reference, bounds, emulation and input families of
tests/optim_refs.py, and the bit models of the bf16 rounding, checked
without a GPU: the reference against FusedAdamW._step_torch and
torch.optim.AdamW in fp64, every family's claimed property, the fp32
emulation of the kernel within 1 x E on the whole GPU matrix, and wrong
kernels (mutations of the reference) at 10 x E or more."""

import numpy as np
import pytest
import torch

from tests import optim_refs as orf
from tests.optim_refs import B1, B2, BF16, EPS, F32, F64, LR, WD

def _note(worst, key, ratios):
    for name, r in ratios.items():
        slot = worst.setdefault(name, {})
        slot[key] = max(slot.get(key, 0.0), r)


# ---------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------
class _Group:
    """what _step_torch touches of a FlatParamGroup, in fp64"""

    def __init__(self, master, grad):
        self.master_arena = master.clone()
        self.param_arena = self.master_arena
        self.grad_arena = grad
        self.state = {}

    def sync_master_to_params(self):
        pass


def test_ref_equals_step_torch_fp64():
    from easyparallellibrary_amd.runtime.optim import FusedAdamW
    gen = torch.Generator().manual_seed(3)
    n = 1000
    p = torch.randn(n, generator=gen, dtype=F64)
    grp = _Group(p, None)
    opt = FusedAdamW([grp], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    assert grp.state["exp_avg"].dtype == F64
    m, v = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    worst = 0.0
    for step in (1, 2, 3):
        # _step_torch reads the gradient as fp32: give it fp32 values
        g = (torch.randn(n, generator=gen) * 64).to(F64)
        grp.grad_arena = g
        opt.step_count = step
        opt._step_torch(grp, 1.0 / 64)
        ref = orf.adamw_ref(p, g, m, v, LR, B1, B2, EPS, WD, step, 1.0 / 64)
        for got, want in ((grp.master_arena, ref["master"]),
                          (grp.state["exp_avg"], ref["m"]),
                          (grp.state["exp_avg_sq"], ref["v"])):
            worst = max(worst, float(((got - want).abs() /
                                      want.abs().clamp_min(1e-3)).max()))
        p, m, v = ref["master"], ref["m"], ref["v"]
    print("ref vs _step_torch fp64: worst rel %.3g" % worst)
    assert worst <= 1e-12


def test_ref_equals_torch_adamw_fp64():
    gen = torch.Generator().manual_seed(4)
    n = 1000
    w = torch.nn.Parameter(torch.randn(n, generator=gen, dtype=F64))
    opt = torch.optim.AdamW([w], lr=LR, betas=(B1, B2), eps=EPS,
                            weight_decay=WD)
    p = w.detach().clone()
    m, v = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    worst = 0.0
    for step in (1, 2, 3):
        g = torch.randn(n, generator=gen, dtype=F64)
        w.grad = g.clone()
        opt.step()
        ref = orf.adamw_ref(p, g, m, v, LR, B1, B2, EPS, WD, step, 1.0)
        worst = max(worst, float(((w.detach() - ref["master"]).abs() /
                                  ref["master"].abs().clamp_min(1e-3)).max()))
        p, m, v = ref["master"], ref["m"], ref["v"]
    print("ref vs torch.optim.AdamW fp64: worst rel %.3g" % worst)
    assert worst <= 1e-12


def test_hyper_parameters_are_fp32():
    for x in (B1, B2, EPS, LR, WD, orf.f32(1.0 / 3.0)):
        assert orf.f32(x) == x
    for b in (B1, B2):      # 1 - beta is exact in fp32
        assert float(torch.tensor(1.0) - torch.tensor(b, dtype=F32)) == 1 - b


# ---------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("grad_bf16", [True, False])
def test_family_properties(grad_bf16):
    n = 12345
    for case in orf.CASES:
        for step in orf.STEPS:
            inp = orf.adamw_inputs(case, n, grad_bf16)
            assert inp["grad"].dtype == (BF16 if grad_bf16 else F32)
            for k in ("master", "m", "v"):
                assert inp[k].dtype == F32 and inp[k].numel() == n
            assert bool((inp["v"] >= 0).all())
            ref, e = orf.adamw_reference_of(inp, LR, step)
            p64 = inp["master"].to(F64)
            fam, var = case
            if fam == "zero_master":
                assert not inp["master"].any()
                assert inp["wd"] == (0.0 if var == "wd0" else WD)
                assert torch.equal(ref["master"], -LR * ref["update"])
            elif fam == "small_master":
                assert float(inp["master"].abs().max()) < 2.0 ** -17
            elif fam == "big_master":
                assert bool((inp["master"].abs() == 1024).all())
                assert inp["wd"] == 0.0
                # a quarter ulp above 2^10 is half an ulp below it
                move = LR * (ref["update"].abs() + e["update"])
                assert float(move.max()) < 2.0 ** -15
                assert torch.equal(ref["master"].to(F32), inp["master"])
            elif fam == "cancel_m":
                assert bool((ref["m"].abs() <= 2.0 ** -20 * ref["a"].abs())
                            .all())
                assert bool((e["m"] > 4 * ref["m"].abs()).all())
            elif fam == "zero_grad":
                assert not inp["grad"].any()
                if var == "all":
                    assert not inp["m"].any() and not inp["v"].any()
                    assert not ref["update"].any()
                    assert torch.equal(ref["master"],
                                       p64 - LR * (WD * p64))
                else:
                    assert bool((inp["v"] > 0).all())
            elif fam == "tiny_grad":
                g2 = (1 - B2) * inp["grad"].to(F64) ** 2
                live = inp["grad"] != 0
                assert bool((g2[live] < 2.0 ** -126).all())
                assert bool((ref["root"] < 1e-6 * EPS).all())
                assert not inp["master"][0::2].any()
            elif fam == "scaled":
                gs = inp["grad"].to(F64) * inp["inv_scale"]
                assert 3.0 < float(gs.abs().max()) < 8.0
                # an unscale that is skipped or doubled is off by more
                # than 2^16 for the powers of two, by 3 for the third
                assert inp["inv_scale"] in (2.0 ** -44, 2.0 ** -16,
                                            orf.f32(1.0 / 3.0))


def test_matrix_covers_the_issue():
    mat = orf.adamw_matrix()
    at = [c for c in mat if c[0] == 12345]
    assert {(c[1], c[2]) for c in at} == {
        (case, s) for case in orf.CASES for s in orf.STEPS}
    for n in (7, 8, "slice"):
        assert {c[4:] for c in mat if c[0] == n} == set(orf.INSTANCES)
    assert {c[4:] for c in at} == set(orf.INSTANCES)
    assert any(c[3] == 0.0 for c in at) and any(c[3] == LR for c in at)
    assert orf.BIG_N % 8 == 5 and orf.BIG_N // 8 == 256 * 4096 + 1


# ---------------------------------------------------------------------------
# emulation within 1 x E
# ---------------------------------------------------------------------------
def _emulated(inp, lr, step, fused, inv_bias=None):
    return orf.adamw_emulate(inp["master"], inp["grad"], inp["m"], inp["v"],
                             lr, B1, B2, EPS, inp["wd"], step,
                             inp["inv_scale"], fused, inv_bias)


def test_emulation_within_bounds_on_gpu_matrix():
    worst = {}
    for n, case, step, lr, gbf, with_param in orf.adamw_matrix():
        size = orf.SLICE[2] - orf.SLICE[1] if n == "slice" else n
        inp = orf.adamw_inputs(case, size, gbf)
        ref, e = orf.adamw_reference_of(inp, lr, step)
        for fused in (False, True):
            got = _emulated(inp, lr, step, fused)
            if lr == 0.0:
                assert orf.same_bits(got["master"], inp["master"])
                assert case == ("zero_grad", "all") or \
                    not torch.equal(got["m"], inp["m"])
            if case[0] == "big_master":
                assert orf.same_bits(got["master"], inp["master"])
            r = orf.adamw_judge(got, ref, e)
            _note(worst, orf.case_name(case), r)
            assert all(x <= 1.0 for x in r.values()), (n, case, step, lr, r)
    inp, ref, e = orf.adamw_big_case()
    for fused in (False, True):
        r = orf.adamw_judge(_emulated(inp, LR, orf.BIG_STEP, fused), ref, e)
        _note(worst, "big_n", r)
        assert all(x <= 1.0 for x in r.values()), r
    print("adamw emulation worst err/E: " + orf.format_worst(worst))
    for name in ("m", "v", "master", "param"):
        print("adamw emulation worst err/E %s: %.3f" %
              (name, max(worst[name].values())))


# ---------------------------------------------------------------------------
# wrong kernels
# ---------------------------------------------------------------------------
def _mutant(name, inp, lr, step):
    """the reference with one thing wrong, rounded to the kernel's output
    types"""
    p, g0 = inp["master"].to(F64), inp["grad"].to(F64)
    m0, v0 = inp["m"].to(F64), inp["v"].to(F64)
    s, wd = inp["inv_scale"], inp["wd"]
    g = g0 * s * (s if name == "scale_twice" else 1.0)
    if name == "coupled_l2":
        g = g + wd * p
    bm = B2 if name == "beta2_for_m" else B1
    m = bm * m0 + (1 - bm) * g
    gv = g0 if name == "v_unscaled" else g
    v = B2 * v0 + (1 - B2) * gv * gv
    t = step - 1 if name == "bias_prev_step" else step
    i1, i2 = (1.0, 1.0) if name == "no_bias" else (
        1.0 / (1.0 - B1 ** t) if t else float("inf"),
        1.0 / (1.0 - B2 ** t) if t else float("inf"))
    if name == "eps_inside":
        q = m * i1 / (v * i2 + EPS).sqrt()
    else:
        q = m * i1 / ((v * i2).sqrt() + EPS)
    if name == "coupled_l2":
        new = p - lr * q
    elif name == "decay_at_new_p":
        new = p - lr * q
        new = new - lr * wd * new
    else:
        new = p - lr * (q + wd * p)
    out = dict(m=m.to(F32), v=v.to(F32), master=new.to(F32))
    n = p.numel()
    skip = {"tail_skipped": slice(n - n % 8, n),
            "second_pass_skipped": slice(min(n, orf.GRID_PASS), n)}.get(name)
    if skip is not None:
        for k in ("m", "v", "master"):
            out[k][skip] = inp[k][skip]
    out["param"] = out["master"].to(BF16)
    if name == "param_pre_update":
        out["param"] = inp["master"].to(BF16)
    elif name == "param_truncated":
        out["param"] = (out["master"].view(torch.int32) >> 16).to(
            torch.int16).view(BF16)
    if skip is not None:
        out["param"][skip] = float("nan")   # the pre-filled sentinel stays
    return out


MUTANTS = ("no_bias", "bias_prev_step", "eps_inside", "coupled_l2",
           "v_unscaled", "scale_twice", "beta2_for_m", "decay_at_new_p",
           "param_pre_update", "param_truncated", "tail_skipped")


def test_criterion_rejects_wrong_kernels():
    """each mutant is over 10 x E on some element of some family"""
    best = {name: (0.0, None) for name in MUTANTS}
    for case in orf.CASES:
        for step in orf.STEPS:
            inp = orf.adamw_inputs(case, 12345, False)
            ref, e = orf.adamw_reference_of(inp, LR, step)
            for name in MUTANTS:
                r = max(orf.adamw_judge(_mutant(name, inp, LR, step), ref,
                                        e).values())
                if r > best[name][0]:
                    best[name] = (r, "%s step %d" % (orf.case_name(case),
                                                     step))
    for name in MUTANTS:
        print("mutant %-18s worst err/E %.3g (%s)" % ((name,) + best[name]))
    assert all(best[name][0] >= 10.0 for name in MUTANTS), best


def test_criterion_rejects_skipped_second_pass():
    inp, ref, e = orf.adamw_big_case()
    good = dict(m=ref["m"].to(F32), v=ref["v"].to(F32),
                master=ref["master"].to(F32))
    good["param"] = good["master"].to(BF16)
    r = orf.adamw_judge(good, ref, e)
    assert max(r.values()) <= 1.0, r
    bad = {k: t.clone() for k, t in good.items()}
    for k in ("m", "v", "master"):
        bad[k][orf.GRID_PASS:] = inp[k][orf.GRID_PASS:]
    bad["param"][orf.GRID_PASS:] = float("nan")
    r = orf.adamw_judge(bad, ref, e)
    print("mutant second_pass_skipped worst err/E %.3g" % max(r.values()))
    assert max(r.values()) >= 10.0


def test_parent_host_bias_correction():
    """inv_bias from fp32 powf, as the host code computed it before: the
    err / E of the emulated kernel on zero_master at steps 2-5, against
    the same emulation with the once-rounded value.  The bound's inv_bias
    term (one rounding each) does not cover the fp32 arithmetic."""
    over = 0
    for step in (1, 2, 3, 4, 5, 10, 1000):
        ib = (orf.inv_bias_powf(B1, step), orf.inv_bias_powf(B2, step))
        rel2 = abs(ib[1] / orf.inv_bias64(B2, step) - 1) / orf.U_F32
        line = "step %d inv_bias2 error %.1f u;" % (step, rel2)
        for var in ("wd0", "wd"):
            inp = orf.adamw_inputs(("zero_master", var), 12345, False)
            ref, e = orf.adamw_reference_of(inp, LR, step)
            for fused in (False, True):
                old = orf.adamw_judge(_emulated(inp, LR, step, fused, ib),
                                      ref, e)["master"]
                new = orf.adamw_judge(_emulated(inp, LR, step, fused),
                                      ref, e)["master"]
                line += " %s fused%d parent %.3f fixed %.3f;" % (
                    var, fused, old, new)
                assert new <= 1.0
                over += (2 <= step <= 5) and old > 1.0
        print(line)
    assert over > 0


# ---------------------------------------------------------------------------
# sqnorm bound
# ---------------------------------------------------------------------------
def test_sqnorm_launch_counts():
    assert orf.sqnorm_launch(0) == (1, 0)
    assert orf.sqnorm_launch(257) == (2, 1)
    assert orf.sqnorm_launch(1024 * 256) == (1024, 1)
    assert orf.sqnorm_launch(1024 * 256 + 77) == (1024, 2)
    # sequential fp32 summation in the kernel's shape stays inside
    gen = torch.Generator().manual_seed(0)
    for n in (255, 777, 1024 * 256 + 77):
        x = torch.randn(n, generator=gen)
        blocks, _ = orf.sqnorm_launch(n)
        pad = torch.zeros(-(-n // (blocks * 256)) * blocks * 256)
        pad[:n] = x * x
        acc = torch.zeros(blocks * 256)
        for row in pad.view(-1, blocks * 256):
            acc = acc + row
        per_block = acc.view(blocks, 256)
        for _ in range(8):
            half = per_block.shape[1] // 2
            per_block = per_block[:, :half] + per_block[:, half:]
        total = torch.zeros(())
        for b in per_block.reshape(-1):
            total = total + b
        ref = orf.sqnorm_ref(x)
        r = abs(float(total) - ref) / orf.sqnorm_bounds(n, ref)
        print("sqnorm emulation n %d: err/E %.3g" % (n, r))
        assert r <= 1.0


# ---------------------------------------------------------------------------
# f2bf
# ---------------------------------------------------------------------------
def test_f2bf_models():
    bits = orf.all_bit_patterns()
    assert bits.size == 65536 * len(orf.LOW_HALVES)
    want = orf.bf16_bits(orf.f32_from_bits(bits).to(BF16))
    nan = (bits & 0x7fffffff) > 0x7f800000
    fixed, parent = orf.f2bf_fixed(bits), orf.f2bf_parent(bits)
    assert np.array_equal(fixed[~nan], want[~nan])
    assert np.array_equal(parent[~nan], fixed[~nan])
    assert bool(((fixed[nan] & 0x7fff) > 0x7f80).all())
    assert bool(((want[nan] & 0x7fff) > 0x7f80).all())
    pats = np.asarray(orf.NAN_PATTERNS, dtype=np.uint32)
    assert orf.f2bf_parent(pats).tolist() == [0x8000, 0x0000, 0x8000, 0x7f80]
    lost = int(((parent[nan] & 0x7fff) <= 0x7f80).sum())
    print("f2bf parent: %d of %d NaN patterns come out finite or Inf" %
          (lost, int(nan.sum())))
    assert lost > 0
    assert orf.f2bf_fixed(np.asarray([0x7f7fffff], np.uint32))[0] == 0x7f80
