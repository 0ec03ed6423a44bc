"""The grouped attention kernels (attention_gqa.hip, attention_band.hip,
attention_interval.hip) on the cases and joint input families of
attn_group_cases.py: direct _C calls against the fp64 reference under the
brute-force mask, B = 2 with different bounds per sample.

q / out / dout / dq come from a guarded layout of kernel_refs.attn_layout
with H heads, k / v / dk / dv from one with Hkv heads, lse and delta from
attn_flat; every buffer is pre-filled with the NaN sentinel, and so are the
rows >= len of q, k, v, dout.  Every case asserts

* rows < len of out, dq, dk, dv within 2 E, of lse and delta within E
  (kernel_refs.ATTN_FACTOR; delta against the kernel's own out);
* rows >= len of out, dq, dk, dv, lse exactly zero, everything else finite;
* no write outside the addressed elements of any buffer;
* a second run with equal bits; with lengths three more, whose padding
  holds zeros, +-3e38 and the values the builder left there (one of them a
  lure on key len), all with the bits of the first.

test_attention_group_refs_cpu.py proves the criterion on the same cases.
``GROUP-RATIO`` lines carry the worst err / E per output (docs/testing.md)."""

import pytest
import torch

from tests import attn_group_cases as gc
from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16
BIG = 3.0e38
PADDED = ("out", "dq", "dk", "dv", "lse")


def device_bounds(kernel, case, b=gc.B):
    """what the op hands the kernels: band_bounds / interval_bounds on the
    device ([1, S] without documents), prefix-LM written directly"""
    from easyparallellibrary_amd.ops.attention import (
        band_bounds, interval_bounds)
    seq, ids, window, _, _ = gc.case_mask(kernel, case, b)
    if kernel in ("gqa", "gqa_causal"):
        return ()
    if case == "prefix_lm":
        return tuple(t.int().contiguous().cuda()
                     for t in gc.prefix_bounds(seq))
    make = band_bounds if kernel == "band" else interval_bounds
    return make(None if ids is None else ids.cuda(), window, seq, "cuda")


class Run:
    """one forward + backward through the bindings, results on the CPU.
    pad: what the rows >= len of q, k, v, dout hold on the device ("nan":
    the sentinel the buffers are pre-filled with, "zero", "big": +-3e38,
    "keep": what the builder generated)"""

    def __init__(self, kernel, inp, bounds, lens=None, layout="plain",
                 pad="nan"):
        from easyparallellibrary_amd import _C
        q, k = inp[0], inp[1]
        b, h, seq, d = q.shape
        hkv = k.shape[1]
        layq = kr.attn_layout(layout, b, h, seq, d, "cuda")
        laykv = kr.attn_layout(layout, b, hkv, seq, d, "cuda")
        for lay, key, t in ((layq, "q", inp[0]), (laykv, "k", inp[1]),
                            (laykv, "v", inp[2]), (layq, "dout", inp[3])):
            t = t.to(BF16).cuda()
            for i in range(b):
                n = seq if lens is None or pad == "keep" else lens[i]
                lay[key][i, :, :n].copy_(t[i, :, :n])
                if pad == "zero":
                    lay[key][i, :, n:].zero_()
                elif pad == "big":
                    sign = 1.0 - 2.0 * (torch.arange(seq - n) % 2)
                    lay[key][i, :, n:] = (BIG * sign).to(BF16).cuda()[
                        None, :, None]
        flat = {name: kr.attn_flat(b * h * seq, torch.float32, "cuda")
                for name in ("lse", "delta")}
        sl = None if lens is None else torch.tensor(
            lens, dtype=torch.int32, device="cuda")
        scale = d ** -0.5
        fwd = (layq["q"], laykv["k"], laykv["v"], layq["out"],
               flat["lse"].view, scale)
        bwd = (layq["q"], laykv["k"], laykv["v"], layq["out"], layq["dout"],
               flat["lse"].view, flat["delta"].view, layq["dq"], laykv["dk"],
               laykv["dv"], scale)
        if kernel in ("gqa", "gqa_causal"):
            causal = kernel == "gqa_causal"
            _C.attn_fwd_gqa(*fwd, causal, sl)
            _C.attn_bwd_gqa(*bwd, causal, sl)
        elif kernel == "band":
            _C.attn_fwd_band(*fwd, bounds[0], sl)
            _C.attn_bwd_band(*bwd, *bounds, sl)
        else:
            _C.attn_fwd_interval(*fwd, *bounds[:2], sl)
            _C.attn_bwd_interval(*bwd, *bounds, sl)
        torch.cuda.synchronize()
        self.raw = dict(out=layq["out"].cpu(), dq=layq["dq"].cpu(),
                        dk=laykv["dk"].cpu(), dv=laykv["dv"].cpu())
        for name in ("lse", "delta"):
            self.raw[name] = flat[name].view.cpu().reshape(b, h, seq)
        self.got = {name: t.to(F64) for name, t in self.raw.items()}
        self.lens = (seq,) * b if lens is None else tuple(lens)
        # what each layout does not lend to this call stays untouched too
        self.stray = {}
        for tag, bufs in (("q.", layq["buffers"]), ("kv.", laykv["buffers"]),
                          ("", flat)):
            for key, buf in bufs.items():
                self.stray[tag + key] = buf.stray_writes()
        for lay, keys in ((layq, ("k", "v", "dk", "dv")),
                          (laykv, ("q", "dout", "dq", "out"))):
            for key in keys:
                self.stray["unused." + key] = int(
                    (lay["buffers"][key].raw != lay["buffers"][key].sentinel
                     ).sum())


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def differing(a, b):
    """outputs whose bits differ between two runs; delta on the rows
    < len only (the others are unspecified)"""
    bad = []
    for name in kr.ATTN_OUTPUTS:
        x, y = _bits(a.raw[name]), _bits(b.raw[name])
        if name == "delta":
            if any(not torch.equal(x[i, :, :n], y[i, :, :n])
                   for i, n in enumerate(a.lens)):
                bad.append(name)
        elif not torch.equal(x, y):
            bad.append(name)
    return bad


def check(label, run, inp, valid, lens):
    ref, bounds = gc.group_reference(*inp, valid)
    ratios = gc.group_ratios(run.got, ref, bounds, inp[3], lens)
    print("GROUP-RATIO {} {}".format(label, " ".join(
        "{}={:.3f}".format(name, ratios[name]) for name in kr.ATTN_OUTPUTS)))
    bad = ["{} err/E {:.3f} > {}".format(name, r, kr.ATTN_FACTOR[name])
           for name, r in ratios.items() if not r <= kr.ATTN_FACTOR[name]]
    for i, n in enumerate(run.lens):
        for name in kr.ATTN_OUTPUTS:
            if not bool(torch.isfinite(run.got[name][i, :, :n]).all()):
                bad.append("{} sample {}: not finite".format(name, i))
        for name in PADDED:
            if bool(run.got[name][i, :, n:].ne(0).any()):
                bad.append("{} sample {}: padded rows not 0".format(name, i))
    bad += ["{} stray writes in {}".format(n, key)
            for key, n in run.stray.items() if n]
    assert not bad, (label, bad)


def run_case(label, kernel, case, family, d, h, hkv, b=gc.B, layout="plain"):
    seq, _, _, lens, valid = gc.case_mask(kernel, case, b)
    inp = gc.group_inputs(family, seq, d, h, hkv, b, valid, lens=lens)
    bounds = device_bounds(kernel, case, b)
    first = Run(kernel, inp, bounds, lens, layout)
    check(label, first, inp, valid, lens)
    for pad in ("nan",) + (() if lens is None else ("zero", "big", "keep")):
        again = Run(kernel, inp, bounds, lens, layout, pad)
        assert not differing(first, again), (label, pad,
                                             differing(first, again))


@pytest.mark.parametrize("index", range(len(gc.MAIN)), ids=[
    "{}-d{}-h{}kv{}-{}-{}-{}".format(*c, gc.main_family(i), gc.main_layout(i))
    for i, c in enumerate(gc.MAIN)])
def test_group_kernels_against_fp64(index):
    kernel, d, h, hkv, case = gc.MAIN[index]
    family, layout = gc.main_family(index), gc.main_layout(index)
    run_case("main {} d{} h{}/{} {} {} {}".format(
        kernel, d, h, hkv, case, family, layout), kernel, case, family, d, h,
        hkv, layout=layout)


@pytest.mark.parametrize("kernel,b,h,hkv", gc.ORDER)
def test_block_order_with_different_bounds_per_sample(kernel, b, h, hkv):
    """B * Hkv = 9 and 17: block_of / causal_group_bh permute the first
    multiple of eight batch-kv-heads and keep the rest, and every sample
    has bounds (the GQA kernels: a length) of its own"""
    run_case("order {} b{} h{}/{}".format(kernel, b, h, hkv), kernel,
             "order", "peaked", 64, h, hkv, b)


@pytest.mark.parametrize("kernel", ["band", "interval"])
def test_broadcast_bounds_give_the_bits_of_repeated_ones(kernel):
    """a [1, S] bound row against the same row repeated to [B, S]"""
    from easyparallellibrary_amd.ops.attention import (
        band_bounds, interval_bounds)
    seq, d, h, hkv, window = 200, 64, 4, 2, 33
    causal = kernel == "band"
    valid = (gc.band_valid if causal else gc.interval_valid)(
        None, window, seq, [seq] * gc.B)
    inp = gc.group_inputs("edge", seq, d, h, hkv, gc.B, valid)
    one = (band_bounds if causal else interval_bounds)(
        None, window, seq, "cuda")
    assert all(t.shape == (1, seq) for t in one)
    first = Run(kernel, inp, one)
    check("broadcast " + kernel, first, inp, valid, None)
    again = Run(kernel, inp, tuple(t.repeat(gc.B, 1).contiguous()
                                   for t in one))
    assert not differing(first, again), differing(first, again)
