"""Flash attention (csrc/kernels/attention.hip) against the fp64 reference
of kernel_refs.py, with the derived per-element rounding bounds.

Direct _C.attn_fwd / _C.attn_bwd calls on constructed inputs (families
randn / peaked / shifted, B = 2, H = 3) in three memory layouts.  Every
case asserts

* |out - ref| <= 2 E_out and the same for dq, dk, dv; lse within E_lse;
  the delta workspace within E_delta of rowsum(dout o out) - dlse taken
  over the kernel's own bf16 out (kernel_refs.attn_bounds derives the E's,
  test_kernel_refs_cpu.py proves them at 1 x E for the rounding model and
  shows that they reject eleven wrong kernels);
* every result is finite;
* every sentinel outside the addressed elements (row padding, storage
  offset, two guard rows before and after each buffer, guards around lse,
  delta and the mask words) is untouched.

Each case prints its worst err / E per output (``ATTN-RATIO`` lines; the
table in docs/testing.md is made from them).

EPL_ATTN_BWD_TILES and EPL_ATTN_BWD_DBUF are read once per process, so the
environment-selected paths run in fresh child processes, six side by
side, which write their ratios to JSON; the parent applies the same
criterion.
"""

import json
import math
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, REPO)

from tests import kernel_refs as kr  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
B, H = kr.ATTN_B, kr.ATTN_H
SEED = (77 << 32) + 12345      # both philox key words non-zero
GRADS = ("out", "dq", "dk", "dv")


class Run:
    """one forward + backward through the kernels, results on the CPU"""

    def __init__(self, inp, d, causal, layout, thresh=0, seed=SEED,
                 dlse=None, split=True, mask_fill=0):
        from easyparallellibrary_amd import _C
        seq = inp[0].shape[2]
        lay = kr.attn_layout(layout, B, H, seq, d, "cuda")
        for key, t in zip(("q", "k", "v", "dout"), inp):
            lay[key].copy_(t.to(torch.bfloat16))
        flat = {"lse": kr.attn_flat(B * H * seq, torch.float32, "cuda"),
                "delta": kr.attn_flat(B * H * seq, torch.float32, "cuda")}
        mask = None
        if thresh:
            flat["mask"] = kr.attn_flat(B * H * seq * ((seq + 31) // 32),
                                        torch.int32, "cuda")
            mask = flat["mask"].view
            mask.fill_(mask_fill)
        dl = None if dlse is None else dlse.reshape(-1).float().cuda()
        scale = d ** -0.5
        inv_keep = kr.attn_inv_keep(thresh)
        _C.attn_fwd(lay["q"], lay["k"], lay["v"], lay["out"],
                    flat["lse"].view, scale, causal, mask, seed, thresh,
                    inv_keep)
        _C.attn_bwd(lay["q"], lay["k"], lay["v"], lay["out"], lay["dout"],
                    flat["lse"].view, flat["delta"].view, lay["dq"],
                    lay["dk"], lay["dv"], scale, causal, split, mask,
                    inv_keep, dl)
        torch.cuda.synchronize()
        self.raw = {name: lay[name].cpu() for name in GRADS}
        for name in ("lse", "delta"):
            self.raw[name] = flat[name].view.cpu().reshape(B, H, seq)
        self.got = {name: t.to(F64) for name, t in self.raw.items()}
        self.words = None if mask is None else mask.cpu()
        bufs = dict(lay["buffers"], **flat)
        self.stray = {key: buf.stray_writes() for key, buf in bufs.items()}
        self.seq, self.causal = seq, causal

    def keep(self):
        return kr.unpack_keep(self.words, B * H, self.seq).reshape(
            B, H, self.seq, self.seq)

    def valid_bits(self):
        """the keep bits the kernels may use: keys inside the sequence,
        at or below the diagonal when causal"""
        return self.keep()[:, :, kr.attn_valid(self.seq, self.seq,
                                               self.causal)]


class Ref:
    """reference and bounds of one (inputs, mask, dlse), shared between
    the layouts that run it"""

    def __init__(self, inp, d, causal, keep=None, thresh=0, dlse=None):
        q, k, v, dout = inp
        scale = d ** -0.5
        self.dout, self.dlse = dout, dlse
        self.ref = kr.attn_ref(q, k, v, dout, causal, scale, keep,
                               kr.attn_inv_keep(thresh), dlse)
        self.bounds = kr.attn_bounds(self.ref, q, k, v, dout, scale)

    def ratios(self, run):
        res = {}
        for name in kr.ATTN_OUTPUTS:
            want, bound = self.ref[name], self.bounds[name]
            if name == "delta":
                want, bound = kr.attn_delta_ref(self.dout, run.got["out"],
                                                self.dlse)
            res[name] = kr.attn_ratio((run.got[name] - want).abs(), bound)
        return res


def report(setting, label, ratios):
    print("ATTN-RATIO {} {} {}".format(setting, label, " ".join(
        "{}={:.3f}".format(name, ratios[name]) for name in kr.ATTN_OUTPUTS)))


def verdict(run, ratios):
    """the failures of one case, as text (empty: the case passes)"""
    bad = ["{} err/E {:.3f} > {}".format(name, r, kr.ATTN_FACTOR[name])
           for name, r in ratios.items()
           if not r <= kr.ATTN_FACTOR[name]]
    bad += ["{} not finite".format(name) for name, t in run.got.items()
            if not bool(torch.isfinite(t).all())]
    bad += ["{} stray writes in {}".format(n, key)
            for key, n in run.stray.items() if n]
    return bad


def check(setting, label, run, ref):
    ratios = ref.ratios(run)
    report(setting, label, ratios)
    bad = verdict(run, ratios)
    assert not bad, (setting, label, bad)


def layouts_of(seq, index):
    if seq in kr.ATTN_CROSSED_SEQS:
        return kr.ATTN_LAYOUTS
    return (kr.ATTN_LAYOUTS[index % len(kr.ATTN_LAYOUTS)],)


# --------------------------------------------------------------------------
# main matrix, default environment
# --------------------------------------------------------------------------
MAIN = [(d, seq, causal, family)
        for d in kr.ATTN_DIMS for seq in kr.ATTN_SEQS
        for causal in (False, True) for family in kr.ATTN_FAMILIES]


@pytest.mark.parametrize(
    "index", range(len(MAIN)),
    ids=["d{}-s{}-{}-{}".format(d, s, "causal" if c else "full", f)
         for d, s, c, f in MAIN])
def test_main_matrix(index):
    d, seq, causal, family = MAIN[index]
    inp = kr.attn_inputs(family, seq, d, causal)
    ref = Ref(inp, d, causal)
    for layout in layouts_of(seq, index):
        check("main", "d{} s{} causal{} {} {}".format(
            d, seq, int(causal), family, layout),
            Run(inp, d, causal, layout), ref)


# --------------------------------------------------------------------------
# dropout
# --------------------------------------------------------------------------
@pytest.mark.parametrize("thresh", sorted(kr.ATTN_DROP_FAMILY))
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("seq", kr.ATTN_DROP_SEQS)
@pytest.mark.parametrize("d", kr.ATTN_DIMS)
def test_dropout(d, seq, causal, thresh):
    family = kr.ATTN_DROP_FAMILY[thresh]
    inp = kr.attn_inputs(family, seq, d, causal)
    runs = {layout: Run(inp, d, causal, layout, thresh)
            for layout in ("plain", "qkv")}
    bits = runs["plain"].valid_bits()
    # same (B, H, S, seed): the layout does not move a bit
    assert torch.equal(bits, runs["qkv"].valid_bits())
    # keep rate within 5 sigma of 1 - thresh / 256
    p = 1.0 - thresh / 256.0
    sigma = math.sqrt(p * (1.0 - p) / bits.numel())
    rate = float(bits.mean())
    print("keep rate {:.5f} expected {:.5f} sigma {:.2e} n {}".format(
        rate, p, sigma, bits.numel()))
    assert abs(rate - p) <= 5.0 * sigma, (rate, p, sigma)
    # forward and backward against the reference fed the published mask
    ref = Ref(inp, d, causal, runs["plain"].keep(), thresh)
    for layout, run in runs.items():
        check("dropout", "d{} s{} causal{} thresh{} {} {}".format(
            d, seq, int(causal), thresh, family, layout), run, ref)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("seq", kr.ATTN_DROP_SEQS)
def test_dropout_mask_identity(seq, causal):
    inp64 = kr.attn_inputs("randn", seq, 64, causal)
    inp128 = kr.attn_inputs("randn", seq, 128, causal)
    a = Run(inp64, 64, causal, "plain", 128)
    again = Run(inp64, 64, causal, "plain", 128)
    wide = Run(inp128, 128, causal, "qkv", 128)
    other = Run(inp64, 64, causal, "plain", 128, seed=SEED + 1)
    assert torch.equal(a.valid_bits(), again.valid_bits())
    assert torch.equal(a.valid_bits(), wide.valid_bits())
    assert not torch.equal(a.valid_bits(), other.valid_bits())
    # the mask depends on the batch-head and on the row: with 33 or more
    # fair bits in common, equal bits mean a counter that does not count
    per_bh = a.valid_bits().reshape(B * H, -1)
    for i in range(B * H):
        for j in range(i + 1, B * H):
            assert not torch.equal(per_bh[i], per_bh[j]), (i, j)
    keep = a.keep()
    valid = kr.attn_valid(seq, seq, causal)
    # row r against row r + 1 on the keys both may use (those of row r)
    same = ((keep[:, :, :-1] == keep[:, :, 1:]) | ~valid[:-1]).all(dim=-1)
    enough = valid[:-1].sum(dim=-1) >= 33
    assert int(enough.sum()) >= seq - 33
    assert not bool(same[:, :, enough].any())


def _bit_pattern(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", kr.ATTN_DIMS)
def test_dropout_ignores_garbage_bits(d, causal):
    """The forward writes the mask words of visited sub-tiles only, and the
    last word of a row carries bits for keys >= seq: neither may reach a
    result."""
    seq = 200
    inp = kr.attn_inputs("randn", seq, d, causal)
    zeros = Run(inp, d, causal, "plain", 128, mask_fill=0)
    ones = Run(inp, d, causal, "plain", 128, mask_fill=-1)
    assert torch.equal(zeros.valid_bits(), ones.valid_bits())
    if causal:
        # the premise: words beyond the diagonal keep what they held
        w = ones.words.reshape(B * H, seq, -1)
        assert bool((w[:, 0, 1:] == -1).all())
        assert bool((zeros.words.reshape(B * H, seq, -1)[:, 0, 1:] == 0)
                    .all())
    for name in kr.ATTN_OUTPUTS:
        assert torch.equal(_bit_pattern(zeros.raw[name]),
                           _bit_pattern(ones.raw[name])), name
    ref = Ref(inp, d, causal, ones.keep(), 128)
    check("dropout", "d{} s{} causal{} mask-prefilled-ones".format(
        d, seq, int(causal)), ones, ref)


# --------------------------------------------------------------------------
# dlse (ring attention's block merge), alone and with a dropout mask
# --------------------------------------------------------------------------
@pytest.mark.parametrize("thresh", [0, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("seq", kr.ATTN_DLSE_SEQS)
@pytest.mark.parametrize("d", kr.ATTN_DIMS)
def test_dlse(d, seq, causal, thresh):
    dlse = kr.attn_dlse(seq)
    assert float(dlse.abs().min()) > 0
    for i, family in enumerate(kr.ATTN_FAMILIES):
        inp = kr.attn_inputs(family, seq, d, causal)
        run = Run(inp, d, causal, kr.ATTN_LAYOUTS[i], thresh, dlse=dlse)
        keep = run.keep() if thresh else None
        check("dlse", "d{} s{} causal{} thresh{} {}".format(
            d, seq, int(causal), thresh, family),
            run, Ref(inp, d, causal, keep, thresh, dlse))


# --------------------------------------------------------------------------
# combined dK+dV kernel with the delta prep kernel (split_dkdv = False)
# --------------------------------------------------------------------------
@pytest.mark.parametrize("seq", kr.ATTN_COMBINED_SEQS)
def test_combined_dkdv(seq):
    for i, family in enumerate(kr.ATTN_FAMILIES):
        inp = kr.attn_inputs(family, seq, 64, False)
        layout = kr.ATTN_LAYOUTS[(i + seq) % len(kr.ATTN_LAYOUTS)]
        check("combined", "d64 s{} causal0 {} {}".format(seq, family, layout),
              Run(inp, 64, False, layout, split=False),
              Ref(inp, 64, False))


# --------------------------------------------------------------------------
# launch-grid limits: refused before any launch
# --------------------------------------------------------------------------
def _expanded(b, h, seq):
    """[b,h,seq,64] over 64 elements: strides (0,0,0,1), no memory"""
    base = torch.zeros(64, device="cuda", dtype=torch.bfloat16)
    return base.expand(b, h, seq, 64)


@pytest.mark.parametrize("b,h,seq,causal", [
    (65536, 1, 1, False),         # batch*heads on gridDim.y
    (256, 257, 1, False),
    (1, 1, 65536 * 128, True),    # 128-row blocks on gridDim.y
    (1, 1, 65535 * 128 + 1, False)])
def test_grid_limits_are_refused(b, h, seq, causal):
    from easyparallellibrary_amd import _C
    t = _expanded(b, h, seq)
    small = torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError, match="65535"):
        _C.attn_fwd(t, t, t, t, small, 0.125, causal, None, 0, 0, 1.0)
    for split in (True, False):
        with pytest.raises(RuntimeError, match="65535"):
            _C.attn_bwd(t, t, t, t, t, small, small, t, t, t, 0.125, causal,
                        split, None, 1.0, None)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------
# environment-selected tile bodies and staging modes: one child each
# --------------------------------------------------------------------------
SETTINGS = [("new", 0), ("new", 1), ("new", 2), ("new", 3),
            ("legacy", 0), ("legacy", 2)]


def _worker(out_path):
    import easyparallellibrary_amd as epl
    epl.init()
    dbuf = int(os.environ["EPL_ATTN_BWD_DBUF"])
    res = {}
    for d, seq, causal, thresh, family in kr.attn_env_cases(dbuf):
        inp = kr.attn_inputs(family, seq, d, causal)
        run = Run(inp, d, causal, "plain", thresh)
        ref = Ref(inp, d, causal, run.keep() if thresh else None, thresh)
        ratios = ref.ratios(run)
        label = "d{} s{} causal{} thresh{} {}".format(
            d, seq, int(causal), thresh, family)
        res[label] = dict(ratios=ratios, bad=verdict(run, ratios))
    with open(out_path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def env_results(tmp_path_factory):
    """{(tiles, dbuf): {case: {ratios, bad}}} — six children side by side"""
    tmp = tmp_path_factory.mktemp("attn_fp64")
    procs = []
    for tiles, dbuf in SETTINGS:
        env = dict(os.environ)
        env.pop("EPL_ATTN_BWD_TILES", None)
        if tiles == "legacy":
            env["EPL_ATTN_BWD_TILES"] = "legacy"
        env["EPL_ATTN_BWD_DBUF"] = str(dbuf)
        out = tmp / "{}_{}.json".format(tiles, dbuf)
        cmd = [sys.executable]
        if sys.flags.no_user_site:
            cmd.append("-s")
        cmd += [os.path.abspath(__file__), "--worker", str(out)]
        procs.append((tiles, dbuf, out, subprocess.Popen(
            cmd, env=env, cwd=REPO, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT, text=True)))
    res = {}
    for tiles, dbuf, out, p in procs:
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, (tiles, dbuf, log[-3000:])
        with open(out) as f:
            res[(tiles, dbuf)] = json.load(f)
    return res


@pytest.mark.parametrize("tiles,dbuf", SETTINGS)
def test_env_selected_paths(env_results, tiles, dbuf):
    res = env_results[(tiles, dbuf)]
    assert len(res) == len(kr.attn_env_cases(dbuf))
    failures = []
    for label, r in res.items():
        report("{}-dbuf{}".format(tiles, dbuf), label, r["ratios"])
        # the same criterion as in-process, applied to the child's figures
        bad = [name for name, x in r["ratios"].items()
               if not x <= kr.ATTN_FACTOR[name]]
        if bad or r["bad"]:
            failures.append((label, bad, r["bad"]))
    assert not failures, failures


if __name__ == "__main__":
    assert sys.argv[1] == "--worker", sys.argv
    _worker(sys.argv[2])
