"""Flash attention on right-padded batches (per-sample ``seqlens``) against
the fp64 reference of varlen_refs.py, with the unchanged per-element bounds
of kernel_refs.attn_bounds.

Direct _C.attn_fwd / _C.attn_bwd calls, B = 2, H = 3, in the guarded
layouts of kernel_refs.attn_layout.  The padded rows of q, k, v and dout
hold a NaN bit pattern on the device unless a test says otherwise, and
every output buffer is pre-filled with it, so a padded row that reaches a
valid result, or an output row that is not written, shows.  Every case
asserts

* rows < len of out, dq within 2 E, lse within E, delta within E_delta;
  dk, dv within 2 E everywhere;
* rows >= len of out, dq, dk, dv, lse exactly zero (they enter the ratios
  at a bound of zero) and every output finite;
* no write outside the addressed elements.

``ATTN-RATIO varlen...`` lines carry the worst err / E per output (the
table in docs/testing.md is made from them).  The environment-selected
tile bodies and staging modes run in fresh child processes, side by side.
"""

import json
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, REPO)

from tests import kernel_refs as kr  # noqa: E402
from tests import varlen_refs as vr  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
H = kr.ATTN_H
SEED = (77 << 32) + 12345      # both philox key words non-zero
GRADS = ("out", "dq", "dk", "dv")
BIG = 3.0e38                   # finite garbage: P = 0 times this must not
#                                be formed (0 * inf after one more factor)


class Run:
    """one forward + backward through the kernels, results on the CPU.
    lens: per-sample lengths, or None for a dense call; pad: what the rows
    >= len of q, k, v, dout hold on the device ("nan": the sentinel the
    buffers are pre-filled with, "zero", "big": +-3e38)."""

    def __init__(self, inp, d, causal, layout, lens=None, thresh=0,
                 seed=SEED, dlse=None, split=True, mask_fill=0, pad="nan",
                 seqlens=None):
        from easyparallellibrary_amd import _C
        b, _, seq, _ = inp[0].shape
        lay = kr.attn_layout(layout, b, H, seq, d, "cuda")
        for key, t in zip(("q", "k", "v", "dout"), inp):
            t = t.to(torch.bfloat16).cuda()
            for i in range(b):
                n = seq if lens is None else lens[i]
                lay[key][i, :, :n].copy_(t[i, :, :n])
                if pad == "zero":
                    lay[key][i, :, n:].zero_()
                elif pad == "big":
                    sign = 1.0 - 2.0 * (torch.arange(seq - n) % 2)
                    lay[key][i, :, n:] = (BIG * sign).to(
                        torch.bfloat16).cuda()[None, :, None]
        flat = {"lse": kr.attn_flat(b * H * seq, torch.float32, "cuda"),
                "delta": kr.attn_flat(b * H * seq, torch.float32, "cuda")}
        mask = None
        if thresh:
            flat["mask"] = kr.attn_flat(b * H * seq * ((seq + 31) // 32),
                                        torch.int32, "cuda")
            mask = flat["mask"].view
            mask.fill_(mask_fill)
        dl = None if dlse is None else dlse.reshape(-1).float().cuda()
        if seqlens is None and lens is not None:
            seqlens = torch.tensor(lens, dtype=torch.int32, device="cuda")
        scale = d ** -0.5
        inv_keep = kr.attn_inv_keep(thresh)
        if seqlens is None:
            # the positional call of before the argument existed
            _C.attn_fwd(lay["q"], lay["k"], lay["v"], lay["out"],
                        flat["lse"].view, scale, causal, mask, seed, thresh,
                        inv_keep)
            _C.attn_bwd(lay["q"], lay["k"], lay["v"], lay["out"],
                        lay["dout"], flat["lse"].view, flat["delta"].view,
                        lay["dq"], lay["dk"], lay["dv"], scale, causal,
                        split, mask, inv_keep, dl)
        else:
            _C.attn_fwd(lay["q"], lay["k"], lay["v"], lay["out"],
                        flat["lse"].view, scale, causal, mask, seed, thresh,
                        inv_keep, seqlens)
            _C.attn_bwd(lay["q"], lay["k"], lay["v"], lay["out"],
                        lay["dout"], flat["lse"].view, flat["delta"].view,
                        lay["dq"], lay["dk"], lay["dv"], scale, causal,
                        split, mask, inv_keep, dl, seqlens)
        torch.cuda.synchronize()
        self.raw = {name: lay[name].cpu() for name in GRADS}
        for name in ("lse", "delta"):
            self.raw[name] = flat[name].view.cpu().reshape(b, H, seq)
        self.got = {name: t.to(F64) for name, t in self.raw.items()}
        self.words = None if mask is None else mask.cpu()
        bufs = dict(lay["buffers"], **flat)
        self.stray = {key: buf.stray_writes() for key, buf in bufs.items()}
        self.b, self.seq, self.lens = b, seq, lens

    def keep(self):
        return kr.unpack_keep(self.words, self.b * H, self.seq).reshape(
            self.b, H, self.seq, self.seq)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b, lens, names=kr.ATTN_OUTPUTS):
    """outputs whose bit patterns differ between two runs; delta is
    compared on the rows < len only (the others are unspecified)"""
    bad = []
    for name in names:
        x, y = _bits(a.raw[name]), _bits(b.raw[name])
        if name == "delta" and lens is not None:
            for i, n in enumerate(lens):
                if not torch.equal(x[i, :, :n], y[i, :, :n]):
                    bad.append(name)
        elif not torch.equal(x, y):
            bad.append(name)
    return bad


def report(setting, label, ratios):
    print("ATTN-RATIO {} {} {}".format(setting, label, " ".join(
        "{}={:.3f}".format(name, ratios[name]) for name in kr.ATTN_OUTPUTS)))


def verdict(run, ratios):
    """the failures of one case, as text (empty: the case passes)"""
    bad = ["{} err/E {:.3f} > {}".format(name, r, kr.ATTN_FACTOR[name])
           for name, r in ratios.items()
           if not r <= kr.ATTN_FACTOR[name]]
    # delta rows >= len are unspecified; everything else is finite
    bad += ["{} not finite".format(name) for name, t in run.got.items()
            if name != "delta" and not bool(torch.isfinite(t).all())]
    for i, n in enumerate(run.lens):
        if not bool(torch.isfinite(run.got["delta"][i, :, :n]).all()):
            bad.append("delta not finite on valid rows")
        for name in GRADS + ("lse",):
            if bool(_bits(run.raw[name][i, :, n:]).ne(0).any()):
                bad.append("{} sample {}: padded rows not +0".format(name, i))
    bad += ["{} stray writes in {}".format(n, key)
            for key, n in run.stray.items() if n]
    return bad


def check(setting, label, run, exp):
    ratios = exp.ratios(run.got)
    report(setting, label, ratios)
    bad = verdict(run, ratios)
    assert not bad, (setting, label, bad)


def _label(d, seq, lens, causal, *rest):
    return "d{} s{} len{}-{} causal{} {}".format(
        d, seq, lens[0], lens[1], int(causal), " ".join(map(str, rest)))


# --------------------------------------------------------------------------
# main matrix: reference, exact zeros, dense equivalence, padding invariance
# --------------------------------------------------------------------------
@pytest.mark.parametrize(
    "index", range(len(vr.MAIN)),
    ids=["d{}-s{}-len{}_{}-{}".format(d, s, l[0], l[1],
                                      "causal" if c else "full")
         for d, s, l, c in vr.MAIN])
def test_main_matrix(index):
    d, seq, lens, causal = vr.MAIN[index]
    family, layout = vr.main_family(index), vr.main_layout(index)
    inp = kr.attn_inputs(family, seq, d, causal)
    exp = vr.Expected(inp, lens, d, causal)
    run = Run(inp, d, causal, layout, lens)
    check("varlen-main", _label(d, seq, lens, causal, family, layout), run,
          exp)
    # what the padding holds reaches nothing, not even a rounding
    for pad in ("zero", "big"):
        other = Run(inp, d, causal, layout, lens, pad=pad)
        assert not same_bits(run, other, lens), (pad, same_bits(
            run, other, lens))
        assert not verdict(other, exp.ratios(other.got))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("seq", [72, 200, 257])
@pytest.mark.parametrize("d", kr.ATTN_DIMS)
def test_full_lengths_equal_dense(d, seq, causal):
    """seqlens all equal to seq (or beyond it: the kernels clamp): every
    output, the delta workspace and the mask words included, has the bits
    of the call without seqlens"""
    inp = kr.attn_inputs("randn", seq, d, causal)
    for thresh in (0, vr.DROP_THRESH):
        dense = Run(inp, d, causal, "qkv", thresh=thresh)
        for n in (seq, seq + 1000):
            full = Run(inp, d, causal, "qkv", thresh=thresh,
                       seqlens=torch.full((vr.B,), n, dtype=torch.int32,
                                          device="cuda"))
            assert not same_bits(dense, full, None), (thresh, n)
            if thresh:
                assert torch.equal(dense.words, full.words)
            assert not any(full.stray.values()), full.stray


def test_negative_length_is_empty():
    """the clamp's lower end: a negative length is an empty sample"""
    seq, d = 72, 64
    inp = kr.attn_inputs("randn", seq, d)
    a = Run(inp, d, False, "plain", (0, 33))
    b = Run(inp, d, False, "plain", (0, 33), seqlens=torch.tensor(
        [-5, 33], dtype=torch.int32, device="cuda"))
    assert not same_bits(a, b, (0, 33))
    assert not verdict(b, vr.Expected(inp, (0, 33), d, False).ratios(b.got))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("seq,lens", [c for c in vr.CASES if c[1][0] > 0])
@pytest.mark.parametrize("d", kr.ATTN_DIMS)
def test_slice_equivalence(d, seq, lens, causal):
    """rows < len_0 of sample 0 carry the bits of a dense call on the
    [:1, :, :len_0] slice: same tiles, same order, same arithmetic"""
    inp = kr.attn_inputs("randn", seq, d, causal)
    n = lens[0]
    run = Run(inp, d, causal, "plain", lens)
    part = Run([t[:1, :, :n] for t in inp], d, causal, "plain")
    for name in kr.ATTN_OUTPUTS:
        assert torch.equal(_bits(run.raw[name][:1, :, :n]),
                           _bits(part.raw[name])), name


# --------------------------------------------------------------------------
# dropout
# --------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("seq,lens", vr.DROP_CASES)
@pytest.mark.parametrize("d", kr.ATTN_DIMS)
def test_dropout(d, seq, lens, causal):
    inp = kr.attn_inputs("randn", seq, d, causal)
    zeros = Run(inp, d, causal, "plain", lens, vr.DROP_THRESH, mask_fill=0)
    ones = Run(inp, d, causal, "qkv", lens, vr.DROP_THRESH, mask_fill=-1)
    # unwritten words and the bits past the length reach nothing
    assert not same_bits(zeros, ones, lens), same_bits(zeros, ones, lens)
    # the premise: rows >= len keep the words they held
    for i, n in enumerate(lens):
        if n < seq:
            w = ones.words.reshape(vr.B, H, seq, -1)[i, :, n:]
            assert bool((w == -1).all())
    # the bits the kernels used are a fair draw
    lb = vr.lens_b1(lens)
    used = vr.valid_mask(seq, lb, causal) & vr.row_mask(seq, lb)[..., None]
    bits = ones.keep()[used.expand(-1, H, -1, -1)]
    assert torch.equal(bits, zeros.keep()[used.expand(-1, H, -1, -1)])
    p = 1.0 - vr.DROP_THRESH / 256.0
    sigma = (p * (1.0 - p) / bits.numel()) ** 0.5
    assert abs(float(bits.mean()) - p) <= 5.0 * sigma
    # forward and backward against the reference fed the published mask
    for name, run in (("zeros", zeros), ("ones", ones)):
        exp = vr.Expected(inp, lens, d, causal, run.keep(), vr.DROP_THRESH)
        check("varlen-dropout", _label(d, seq, lens, causal, "mask-" + name),
              run, exp)


# --------------------------------------------------------------------------
# dlse, the combined-kernel request, the binding's checks
# --------------------------------------------------------------------------
@pytest.mark.parametrize("d,seq,lens,causal", vr.DLSE_CASES)
def test_dlse(d, seq, lens, causal):
    dlse = kr.attn_dlse(seq)
    assert float(dlse.abs().min()) > 0
    for i, family in enumerate(kr.ATTN_FAMILIES):
        inp = kr.attn_inputs(family, seq, d, causal)
        run = Run(inp, d, causal, kr.ATTN_LAYOUTS[i], lens, dlse=dlse)
        check("varlen-dlse", _label(d, seq, lens, causal, family), run,
              vr.Expected(inp, lens, d, causal, dlse=dlse))


@pytest.mark.parametrize("seq,lens", vr.COMBINED_CASES)
def test_combined_request_runs_split(seq, lens):
    """split_dkdv=False with seqlens: the combined kernel knows no padding,
    so the call takes the split kernels and gives their bits"""
    for i, family in enumerate(kr.ATTN_FAMILIES):
        inp = kr.attn_inputs(family, seq, 64, False)
        layout = kr.ATTN_LAYOUTS[i]
        run = Run(inp, 64, False, layout, lens, split=False)
        check("varlen-combined", _label(64, seq, lens, False, family), run,
              vr.Expected(inp, lens, 64, False))
        assert not same_bits(run, Run(inp, 64, False, layout, lens), lens)


def test_binding_refuses_bad_seqlens():
    from easyparallellibrary_amd import _C
    seq, d = 72, 64
    lay = kr.attn_layout("plain", vr.B, H, seq, d, "cuda")
    for key in ("q", "k", "v", "dout", "out"):
        lay[key].zero_()
    lse = torch.zeros(vr.B * H * seq, device="cuda")
    delta = torch.zeros_like(lse)
    good = torch.tensor([72, 37], dtype=torch.int32, device="cuda")
    bad = {"dtype": good.long(), "must hold": good[:1],
           "one per sample": torch.cat([good, good]),
           "device tensor": good.cpu(),
           "contiguous": torch.stack([good, good], 1)[:, 0]}
    before = {k: lay[k].clone() for k in ("dq", "dk", "dv")}
    for match, sl in bad.items():
        with pytest.raises(RuntimeError, match=match):
            _C.attn_fwd(lay["q"], lay["k"], lay["v"], lay["out"], lse,
                        d ** -0.5, False, None, 0, 0, 1.0, sl)
        with pytest.raises(RuntimeError, match=match):
            _C.attn_bwd(lay["q"], lay["k"], lay["v"], lay["out"],
                        lay["dout"], lse, delta, lay["dq"], lay["dk"],
                        lay["dv"], d ** -0.5, False, True, None, 1.0, None,
                        sl)
    torch.cuda.synchronize()
    # refused before launch: nothing was written
    assert not bool(lay["out"].any())
    for k, t in before.items():
        assert torch.equal(_bits(lay[k]), _bits(t))
    # and the keyword spelling reaches the same kernels
    _C.attn_fwd(lay["q"], lay["k"], lay["v"], lay["out"], lse, d ** -0.5,
                False, None, 0, 0, 1.0, seqlens=good)
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
    for d, seq, lens, causal, thresh, family in vr.env_cases(dbuf):
        inp = kr.attn_inputs(family, seq, d, causal)
        run = Run(inp, d, causal, "plain", lens, thresh)
        exp = vr.Expected(inp, lens, d, causal,
                          run.keep() if thresh else None, thresh)
        ratios = exp.ratios(run.got)
        label = _label(d, seq, lens, causal, "thresh{}".format(thresh),
                       family)
        res[label] = dict(ratios=ratios, bad=verdict(run, ratios))
    with open(out_path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def env_results(tmp_path_factory):
    """{(tiles, dbuf): {case: {ratios, bad}}} — six children side by side"""
    tmp = tmp_path_factory.mktemp("attn_varlen")
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
    assert len(res) == len(vr.env_cases(dbuf))
    failures = []
    for label, r in res.items():
        report("varlen-{}-dbuf{}".format(tiles, dbuf), label, r["ratios"])
        # the same criterion as in-process, applied to the child's figures
        bad = [name for name, x in r["ratios"].items()
               if not x <= kr.ATTN_FACTOR[name]]
        if bad or r["bad"]:
            failures.append((label, bad, r["bad"]))
    assert not failures, failures


if __name__ == "__main__":
    assert sys.argv[1] == "--worker", sys.argv
    _worker(sys.argv[2])
