"""One forward + backward through the attention kernels for any (B, H), in
the guarded layouts of kernel_refs.attn_layout, and the criterion of
test_attention_fp64_gpu.py / test_attention_varlen_gpu.py applied to it.
Shared by test_attention_block_order_gpu.py and
test_attention_dkdv_fused_gpu.py (not a test file).

A dense call is judged as the padded call whose lengths all equal seq:
varlen_refs.Expected is then attn_ref + attn_bounds at the factors of
kernel_refs.ATTN_FACTOR on every row, which is what the dense suite asks.
"""

import torch

from tests import kernel_refs as kr
from tests import varlen_refs as vr

F64 = torch.float64
GRADS = ("out", "dq", "dk", "dv")


class Run:
    """results on the CPU.  lens: per-sample lengths handed to the kernels
    as ``seqlens`` (None: a dense call); the rows >= len of q, k, v, dout
    keep the NaN sentinel the buffers are pre-filled with."""

    def __init__(self, inp, d, causal, layout, lens=None, dlse=None,
                 split=True):
        from easyparallellibrary_amd import _C
        b, h, seq, _ = inp[0].shape
        lay = kr.attn_layout(layout, b, h, seq, d, "cuda")
        for key, t in zip(("q", "k", "v", "dout"), inp):
            t = t.to(torch.bfloat16).cuda()
            for i in range(b):
                n = seq if lens is None else lens[i]
                lay[key][i, :, :n].copy_(t[i, :, :n])
        flat = {"lse": kr.attn_flat(b * h * seq, torch.float32, "cuda"),
                "delta": kr.attn_flat(b * h * seq, torch.float32, "cuda")}
        dl = None if dlse is None else dlse.reshape(-1).float().cuda()
        tail = ()
        if lens is not None:
            tail = (torch.tensor(lens, dtype=torch.int32, device="cuda"),)
        scale = d ** -0.5
        _C.attn_fwd(lay["q"], lay["k"], lay["v"], lay["out"],
                    flat["lse"].view, scale, causal, None, 0, 0, 1.0, *tail)
        _C.attn_bwd(lay["q"], lay["k"], lay["v"], lay["out"], lay["dout"],
                    flat["lse"].view, flat["delta"].view, lay["dq"],
                    lay["dk"], lay["dv"], scale, causal, split, None, 1.0,
                    dl, *tail)
        torch.cuda.synchronize()
        self.raw = {name: lay[name].cpu() for name in GRADS}
        for name in ("lse", "delta"):
            self.raw[name] = flat[name].view.cpu().reshape(b, h, seq)
        self.got = {name: t.to(F64) for name, t in self.raw.items()}
        bufs = dict(lay["buffers"], **flat)
        self.stray = {key: buf.stray_writes() for key, buf in bufs.items()}
        self.lens = tuple(lens) if lens is not None else (seq,) * b


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def differing(a, b):
    """outputs whose bit patterns differ between two runs of the same
    lengths; delta on the rows < len only (the others are unspecified)"""
    bad = []
    for name in kr.ATTN_OUTPUTS:
        x, y = bits(a.raw[name]), bits(b.raw[name])
        if name == "delta":
            if any(not torch.equal(x[i, :, :n], y[i, :, :n])
                   for i, n in enumerate(a.lens)):
                bad.append(name)
        elif not torch.equal(x, y):
            bad.append(name)
    return bad


def verdict(run, ratios):
    """the failures of one case, as text (empty: the case passes)"""
    bad = ["{} err/E {:.3f} > {}".format(name, r, kr.ATTN_FACTOR[name])
           for name, r in ratios.items()
           if not r <= kr.ATTN_FACTOR[name]]
    bad += ["{} not finite".format(name) for name, t in run.got.items()
            if name != "delta" and not bool(torch.isfinite(t).all())]
    for i, n in enumerate(run.lens):
        if not bool(torch.isfinite(run.got["delta"][i, :, :n]).all()):
            bad.append("delta not finite on valid rows")
        for name in GRADS + ("lse",):
            if bool(bits(run.raw[name][i, :, n:]).ne(0).any()):
                bad.append("{} sample {}: padded rows not +0".format(name, i))
    bad += ["{} stray writes in {}".format(n, key)
            for key, n in run.stray.items() if n]
    return bad


def expected(inp, d, causal, lens=None, dlse=None):
    """fp64 reference and bounds; shared by the runs of one input"""
    b, _, seq, _ = inp[0].shape
    return vr.Expected(inp, (seq,) * b if lens is None else lens, d, causal,
                       dlse=dlse)


def check(setting, label, run, exp):
    ratios = exp.ratios(run.got)
    print("ATTN-RATIO {} {} {}".format(setting, label, " ".join(
        "{}={:.3f}".format(name, ratios[name]) for name in kr.ATTN_OUTPUTS)))
    bad = verdict(run, ratios)
    assert not bad, (setting, label, bad)
