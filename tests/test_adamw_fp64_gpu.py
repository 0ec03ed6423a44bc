"""_C.fused_adamw called directly, FusedAdamW on a FlatParamGroup and one
engine step, against the fp64 reference and the derived bounds of
tests/optim_refs.py (1 x E on m, v, master; the bf16 parameter equal to
RNE of the kernel's own master, and within half a bf16 step plus E of the
reference).  Every step is judged against the reference started from the
kernel's own previous state.  Arenas sit in guarded buffers pre-filled
with NaN sentinels; every test prints its worst err / E."""

import pytest
import torch

from tests import kernel_refs as kr
from tests import optim_refs as orf
from tests.optim_refs import B1, B2, BF16, EPS, F32, F64, LR

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from easyparallellibrary_amd import _C
else:
    _C = None

GUARD = 64      # elements: 256 bytes of fp32, 128 of bf16


def dev():
    return torch.device("cuda:0")


class Arenas:
    """master, m, v, grad and (optionally) the bf16 parameter of one case
    in guarded buffers of ``n`` elements; the kernel runs on [lo, hi)."""

    def __init__(self, inp, gbf, with_param, n=None, lo=0, hi=None):
        size = inp["master"].numel()
        n = size if n is None else n
        hi = n if hi is None else hi
        assert hi - lo == size
        self.lo, self.hi = lo, hi
        grad = inp["grad"].to(BF16 if gbf else F32)
        self.buf = {}
        for name, t in (("master", inp["master"]), ("m", inp["m"]),
                        ("v", inp["v"]), ("grad", grad)):
            b = kr.attn_flat(n, t.dtype, dev(), GUARD)
            if n != size:       # live values around the slice
                b.view.copy_(torch.arange(n, dtype=F32).to(t.dtype) + 1)
            b.view[lo:hi].copy_(t)
            self.buf[name] = b
        if with_param:          # stays at the NaN sentinel until written
            self.buf["param"] = kr.attn_flat(n, BF16, dev(), GUARD)
        self.before = {k: b.raw.clone() for k, b in self.buf.items()}

    def view(self, name):
        b = self.buf.get(name)
        return None if b is None else b.view[self.lo:self.hi]

    def run(self, lr, wd, step, inv_scale):
        _C.fused_adamw(self.view("master"), self.view("param"),
                       self.view("grad"), self.view("m"), self.view("v"),
                       lr, B1, B2, EPS, wd, step, inv_scale)
        torch.cuda.synchronize()
        return {k: self.view(k).cpu() for k in ("m", "v", "master", "param")
                if k in self.buf}

    def check_untouched(self):
        """no guard touched, the gradient and everything outside the
        slice keep their bits"""
        for name, b in self.buf.items():
            assert b.stray_writes() == 0, name
            raw, was = b.raw.cpu(), self.before[name].cpu()
            lo, hi = GUARD + self.lo, GUARD + self.hi
            assert torch.equal(raw[:lo], was[:lo]), name
            assert torch.equal(raw[hi:], was[hi:]), name
            if name == "grad":
                assert torch.equal(raw, was)


def _show(label, ratios):
    print("%s: worst err/E %s" % (label, " ".join(
        "%s=%.3f" % kv for kv in sorted(ratios.items()))))


def _matrix_id(c):
    return "%s-%s-s%d-lr%d-g%s-p%d" % (
        c[0], orf.case_name(c[1]), c[2], c[3] != 0,
        "bf16" if c[4] else "f32", c[5])


@pytest.mark.parametrize("cfg", orf.adamw_matrix(), ids=_matrix_id)
def test_adamw_matrix(cfg):
    n, case, step, lr, gbf, with_param = cfg
    if n == "slice":
        total, lo, hi = orf.SLICE
    else:
        total, lo, hi = n, 0, n
    inp = orf.adamw_inputs(case, hi - lo, gbf)
    ref, e = orf.adamw_reference_of(inp, lr, step)
    ar = Arenas(inp, gbf, with_param, total, lo, hi)
    got = ar.run(lr, inp["wd"], step, inp["inv_scale"])
    ar.check_untouched()
    r = orf.adamw_judge(got, ref, e)
    _show(_matrix_id(cfg), r)
    assert all(x <= 1.0 for x in r.values()), r
    if lr == 0.0 or case[0] == "big_master":
        assert orf.same_bits(got["master"], inp["master"])
    if lr == 0.0 and case != ("zero_grad", "all"):
        assert not torch.equal(got["m"], inp["m"])      # the state moves


@pytest.mark.parametrize("gbf,with_param", orf.INSTANCES)
def test_adamw_two_runs_bitwise_equal(gbf, with_param):
    inp = orf.adamw_inputs(("randn", ""), 12345, gbf)
    runs = [Arenas(inp, gbf, with_param).run(LR, inp["wd"], 2, 1.0)
            for _ in range(2)]
    for k in runs[0]:
        assert orf.same_bits(runs[0][k], runs[1][k]), k


# ---------------------------------------------------------------------------
# one vector past a full pass of the 4096-block grid, plus a tail
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    return orf.adamw_big_case()


# +Inf, -Inf, NaN in the vector body, past the first grid pass, in the tail
BAD_AT = (16, 17, 18, orf.GRID_PASS + 1, orf.GRID_PASS + 2,
          orf.GRID_PASS + 7, orf.BIG_N - 5, orf.BIG_N - 3, orf.BIG_N - 1)
BAD_VALUES = (float("inf"), float("-inf"), float("nan")) * 3


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("gbf,with_param", orf.INSTANCES)
def test_adamw_past_one_grid_pass(big, gbf, with_param, poison):
    """8 * 256 * 4096 + 13 elements.  With ``poison`` the gradient holds
    +-Inf and NaN at BAD_AT: exactly those elements of every output are
    non-finite afterwards, every other one meets its bound."""
    inp, ref, e = big
    assert orf.BIG_N - 5 >= (orf.BIG_N // 8) * 8 > orf.GRID_PASS + 7
    grad = inp["grad"].to(BF16 if gbf else F32).clone()
    bad = torch.zeros(orf.BIG_N, dtype=torch.bool)
    if poison:
        idx = torch.tensor(BAD_AT)
        grad[idx] = torch.tensor(BAD_VALUES).to(grad.dtype)
        bad[idx] = True
    ar = Arenas(dict(inp, grad=grad), gbf, with_param)
    got = ar.run(LR, inp["wd"], orf.BIG_STEP, inp["inv_scale"])
    ar.check_untouched()
    for name, t in got.items():
        assert torch.equal(~torch.isfinite(t.float()), bad), name
    r = orf.adamw_judge(got, ref, e, select=~bad)
    _show("big poison%d" % poison, r)
    assert all(x <= 1.0 for x in r.values()), r


@pytest.mark.parametrize("gbf", [True, False])
def test_adamw_writeback_of_master_bit_patterns(gbf):
    """lr = 0, wd = 0, g = 0: p' = p, so the writeback sees the master's
    own bits.  NaNs whose rounding add would carry into the exponent or
    the sign come out as NaN, the largest finite fp32 as +Inf; body and
    tail."""
    pats = list(orf.NAN_PATTERNS) + [0x7f7fffff]
    bits = pats + [0x3f800000] * 11 + pats      # 21: 16 body, 5 tail
    n = len(bits)
    inp = dict(master=orf.f32_from_bits(bits), m=torch.zeros(n),
               v=torch.zeros(n), grad=torch.zeros(n))
    ar = Arenas(inp, gbf, True)
    got = ar.run(0.0, 0.0, 1, 1.0)
    ar.check_untouched()
    p = got["param"].float()
    for at in (0, 16):
        print("param bits %s" % [hex(int(x)) for x in
                                 orf.bf16_bits(got["param"][at:at + 5])])
        assert bool(torch.isnan(p[at:at + 4]).all())
        assert bool(torch.isnan(got["master"][at:at + 4]).all())
        assert float(p[at + 4]) == float("inf")
        assert orf.same_bits(got["master"][at + 4:at + 5],
                             inp["master"][at + 4:at + 5])
    assert bool((p[5:16] == 1.0).all())


# ---------------------------------------------------------------------------
# FusedAdamW on a FlatParamGroup
# ---------------------------------------------------------------------------
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def _group(napply=1):
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.env import Env
    from easyparallellibrary_amd.parallel.dp import FlatParamGroup
    from easyparallellibrary_amd.runtime.optim import FusedAdamW
    Env._instance = None
    epl.init(epl.Config({"optimizer.num_apply_group": napply}))
    g = FlatParamGroup(kr.lamb_params(kr.LAMB_SHAPES, BF16, dev(), 1), dev())
    opt = FusedAdamW([g], **HYPER)
    kr.lamb_fill(g, seed=1, grad_mul=0.0, scale_weights=True)
    assert g.total % 128 == 0 and g.master_arena is not g.param_arena
    return g, opt


def _arenas_of(g):
    return dict(master=g.master_arena, param=g.param_arena,
                m=g.state["exp_avg"], v=g.state["exp_avg_sq"])


def _snapshot(g):
    return {k: t.detach().cpu().clone() for k, t in _arenas_of(g).items()}


def test_apply_groups_bitwise_equal():
    """num_apply_group 1, 3, 7: every chunk boundary is a multiple of 128,
    so no element changes between vector body and tail."""
    snaps = {}
    for napply in (1, 3, 7):
        g, opt = _group(napply)
        for step in (1, 2):
            kr.lamb_fill(g, seed=30 + step, grad_mul=8.0)
            opt.step(grad_scale=8.0)
        torch.cuda.synchronize()
        snaps[napply] = _snapshot(g)
        assert not torch.equal(snaps[napply]["m"],
                               torch.zeros_like(snaps[napply]["m"]))
    for napply in (3, 7):
        for k, t in snaps[1].items():
            assert orf.same_bits(t, snaps[napply][k]), (napply, k)


class _NoComm:
    def join(self):
        pass


def test_eager_apply_slices_equal_one_step():
    g1, opt1 = _group()
    kr.lamb_fill(g1, seed=31, grad_mul=8.0)
    opt1.step(grad_scale=8.0)
    torch.cuda.synchronize()
    want = _snapshot(g1)
    g2, opt2 = _group()
    kr.lamb_fill(g2, seed=31, grad_mul=8.0)
    torch.cuda.synchronize()
    n = g2.total
    cuts = [0, n // 3 // 128 * 128, 2 * n // 3 // 128 * 128, n]
    opt2.begin_eager(8.0)
    for i in (1, 2, 0):
        opt2.eager_apply(g2, cuts[i], cuts[i + 1], _NoComm())
    opt2.step()     # fences the apply stream
    torch.cuda.synchronize()
    got = _snapshot(g2)
    assert opt2.step_count == opt1.step_count == 1
    for k, t in want.items():
        assert orf.same_bits(t, got[k]), k


def _judge_group_step(before, grad, after, opt, step, grad_scale):
    """one step of the optimizer's kernel against the reference at the
    optimizer's own doubles rounded to fp32 (what the binding passes)"""
    f = orf.f32
    lr, eps = f(opt.lr), f(opt.eps)
    ref = orf.adamw_ref(before["master"].to(F64), grad.to(F64),
                        before["m"].to(F64), before["v"].to(F64), lr,
                        f(opt.beta1), f(opt.beta2), eps,
                        f(opt.weight_decay), step, f(1.0 / grad_scale))
    assert (f(opt.beta1), f(opt.beta2), eps, lr) == (B1, B2, EPS, LR)
    e = orf.adamw_bounds(ref, lr, eps)
    got = dict(after)
    if got["param"].dtype != BF16:
        got["param"] = None
    return orf.adamw_judge(got, ref, e)


def test_fused_adamw_three_steps_hold_single_step_bounds():
    g, opt = _group(3)
    for step in (1, 2, 3):
        kr.lamb_fill(g, seed=40 + step, grad_mul=8.0)
        torch.cuda.synchronize()
        before, grad = _snapshot(g), g.grad_arena.cpu().clone()
        opt.step(grad_scale=8.0)
        torch.cuda.synchronize()
        r = _judge_group_step(before, grad, _snapshot(g), opt, step, 8.0)
        _show("FusedAdamW step %d" % step, r)
        assert all(x <= 1.0 for x in r.values()), (step, r)
    assert opt.step_count == 3


# ---------------------------------------------------------------------------
# the engine's clip folded into grad_scale
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "amp_o1"])
def test_engine_clip_and_unscale(mode):
    """max_grad_norm 0.5, two micro-batches; bf16 parameters (loss scale
    1), and fp32 parameters under AMP O1 fp16 with the fixed loss scale
    128.  The grad_scale handed to the optimizer is num_micro_batch *
    loss_scale * gnorm / max_norm with gnorm from the fp64 norm of the
    recorded gradient arena: sqnorm's relative bound, halved by the square
    root, plus the fp32 square root (C_SQRT) and one rounding of the
    accumulator."""
    import torch.nn as nn
    import easyparallellibrary_amd as epl
    max_norm, nmb = 0.5, 2
    conf = {"optimizer.max_grad_norm": max_norm,
            "pipeline.num_micro_batch": nmb}
    loss_scale = 1.0
    if mode == "amp_o1":
        conf.update({"amp.level": "O1", "amp.dtype": "fp16",
                     "amp.loss_scale": "128"})
        loss_scale = 128.0
    epl.init(epl.Config(conf))
    torch.manual_seed(5)
    with epl.replicate(device_count=1):
        model = nn.Sequential(nn.Linear(64, 96), nn.ReLU(),
                              nn.Linear(96, 10))
    engine = epl.Engine(model, loss_fn=nn.MSELoss(), optimizer="adamw",
                        lr=1e-3,
                        dtype=BF16 if mode == "bf16" else F32)
    assert engine.amp.loss_scale == loss_scale
    fg = engine.flat_groups[0]
    opt = engine.optimizer
    rec = []
    inner = opt.step

    def recording_step(grad_scale=1.0):
        torch.cuda.synchronize()
        rec.append(dict(before=_snapshot(fg), grad=fg.grad_arena.cpu().clone(),
                        scale=grad_scale))
        inner(grad_scale=grad_scale)
        torch.cuda.synchronize()
        rec[-1]["after"] = _snapshot(fg)

    opt.step = recording_step
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(16, 64, generator=gen).to(engine.device, engine.dtype)
    y = (torch.randn(16, 10, generator=gen) * 4).to(engine.device,
                                                    engine.dtype)
    for step in (1, 2):
        engine.train_step(x, y)
        r = rec[-1]
        base = nmb * loss_scale
        gnorm64 = float(r["grad"].to(F64).norm()) / base
        assert gnorm64 > 2 * max_norm, gnorm64         # the clip is active
        want = base * max(1.0, gnorm64 / max_norm)
        rel = orf.sqnorm_bounds(fg.total, 1.0) / 2 + orf.C_SQRT + orf.U_F32
        err = abs(r["scale"] - want) / want
        print("%s step %d: gnorm %.4g grad_scale %.6g, err/E %.3g" %
              (mode, step, gnorm64, r["scale"], err / rel))
        assert err <= rel
        ratios = _judge_group_step(r["before"], r["grad"], r["after"], opt,
                                   step, r["scale"])
        _show("%s step %d" % (mode, step), ratios)
        assert all(v <= 1.0 for v in ratios.values()), ratios
        assert ("param_rne" in ratios) == (mode == "bf16")
    assert len(rec) == 2 and opt.step_count == 2
