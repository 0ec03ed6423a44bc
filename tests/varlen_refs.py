"""Padded-batch (per-sample length) flash attention: reference, rounding
model, criterion and case lists shared by test_varlen_refs_cpu.py and
test_attention_varlen_gpu.py.  Everything numeric comes from
kernel_refs.py (attn_ref with a key mask, attn_bounds unchanged).

Semantics under test: sample b has len_b = clamp(seqlens[b], 0, seq) valid
leading tokens.  Query i < len_b attends keys j < len_b (j <= i when
causal); rows >= len_b of out, dq, dk, dv and lse are exact zeros; delta
rows >= len_b are unspecified; nothing at a valid position depends on what
the padding holds.

The reference feeds attn_ref the mask valid[b,0,i,j] = j < len_b (& j <= i)
and a dout that is zero on rows >= len_b, so its dk / dv are zero on
padded key rows and the padded query rows contribute nothing.  An empty
sample runs as length 1 in the reference and is ignored there; the
criterion wants all of its outputs zero.
"""

import torch

from tests import kernel_refs as kr

F64 = torch.float64
B, H = kr.ATTN_B, kr.ATTN_H

# (seq, (len_0, len_1)): the tile edges 31-33, 63-65, 127-129, 256/257,
# whole 128-row blocks past the length, the empty and the one-token sample
CASES = ((72, (72, 37)), (72, (1, 64)), (72, (0, 33)),
         (200, (129, 200)), (200, (128, 63)), (200, (65, 127)),
         (257, (257, 100)), (257, (31, 256)), (257, (32, 129)),
         (257, (0, 1)))
MAIN = [(d, seq, lens, causal) for d in kr.ATTN_DIMS
        for seq, lens in CASES for causal in (False, True)]
DROP_THRESH = 128
DROP_CASES = ((200, (129, 63)), (257, (100, 257)))
# (d, seq, lens, causal): one non-zero dlse case per head dim
DLSE_CASES = ((64, 200, (128, 63), False), (128, 257, (31, 256), True))
COMBINED_CASES = ((72, (0, 33)), (200, (65, 127)))
ENV_CASES = ((200, (129, 200)), (200, (65, 127)),
             (257, (257, 100)), (257, (32, 129)))


def main_family(index):
    return kr.ATTN_FAMILIES[index % len(kr.ATTN_FAMILIES)]


def main_layout(index):
    # co-prime strides, so every (family, layout) pair turns up
    return kr.ATTN_LAYOUTS[(index // 2) % len(kr.ATTN_LAYOUTS)]


def env_cases(dbuf):
    """(d, seq, lens, causal, thresh, family) of one EPL_ATTN_BWD_DBUF
    child: d128 stages directly, so it runs in the dbuf-0 children only"""
    dims = kr.ATTN_DIMS if dbuf == 0 else (64,)
    cases = [(d, seq, lens, causal, thresh)
             for d in dims for seq, lens in ENV_CASES
             for causal in (False, True) for thresh in (0, DROP_THRESH)]
    return [c + (kr.ATTN_FAMILIES[i % len(kr.ATTN_FAMILIES)],)
            for i, c in enumerate(cases)]


def lens_b1(lens):
    """[B,1] int64 from a sequence of B lengths"""
    return torch.as_tensor(lens, dtype=torch.int64).reshape(-1, 1)


def valid_mask(seq, lbh, causal):
    """valid[b,h,i,j] = j < lbh[b,h] (& j <= i); lbh is [B,1] or [B,H]"""
    j = torch.arange(seq)
    valid = (j[None, None, None, :] < lbh[:, :, None, None]).expand(
        -1, -1, seq, -1)
    if causal:
        valid = valid & (j[None, :] <= j[:, None])
    return valid


def row_mask(seq, lbh):
    """rows[b,h,i] = i < lbh[b,h]"""
    return torch.arange(seq)[None, None, :] < lbh[:, :, None]


def cpu_keep(seq, thresh, seed=0):
    """Bernoulli keep bits at the kernels' rate 1 - thresh/256"""
    if not thresh:
        return None
    gen = torch.Generator().manual_seed(1900 + seed + seq + thresh)
    u = torch.rand(B, H, seq, seq, generator=gen, dtype=F64)
    return (u >= thresh / 256.0).to(F64)


def _emulate(q, k, v, dout, scale, keep, inv_keep, dlse, valid):
    """kernel_refs.attn_emulate (the kernels' bf16 roundings) under a key
    mask"""
    rnd = kr.bf16_round
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    sm = s.masked_fill(~valid, float("-inf"))
    mx = sm.max(dim=-1, keepdim=True).values
    e = torch.exp(sm - mx)
    l = e.sum(dim=-1, keepdim=True)
    lse = (mx + l.log()).squeeze(-1)
    kf = 1.0 if keep is None else keep * inv_keep
    out = rnd(torch.matmul(rnd(e * kf), v) / l)
    dl = torch.zeros_like(lse) if dlse is None else dlse
    delta = (dout * out).sum(dim=-1) - dl
    p = torch.exp(sm - lse.unsqueeze(-1))
    pd = rnd(p * kf)
    dp = torch.matmul(dout, v.transpose(-1, -2)) * kf
    ds = rnd(p * (dp - delta.unsqueeze(-1)) * scale)
    return dict(out=out, lse=lse, delta=delta,
                dq=rnd(torch.matmul(ds, k)),
                dk=rnd(torch.matmul(ds.transpose(-1, -2), q)),
                dv=rnd(torch.matmul(pd.transpose(-1, -2), dout)))


def model(inp, lbh, causal, scale, keep=None, inv_keep=1.0, dlse=None,
          emulate=False, key_lbh=None, zero_dout=True, zero_rows=True,
          keep_causal=True):
    """The padded-batch kernels as a function of fp64 inputs: attn_ref (or
    the rounding model) under the length mask, dout and dlse zeroed on the
    padded rows, the padded rows of out / lse / dq zeroed.  lbh: [B,1] or
    [B,H] lengths >= 1.  The remaining arguments turn it into the wrong
    kernels of the mutation tests: another key bound (key_lbh), padded
    query rows left in the backward (zero_dout=False), padded output rows
    left at their dense value (zero_rows=False), the causal bound dropped
    (keep_causal=False)."""
    q, k, v, dout = inp
    seq = q.shape[2]
    valid = valid_mask(seq, lbh if key_lbh is None else key_lbh,
                       causal and keep_causal)
    rows = row_mask(seq, lbh).to(F64)
    dz, dlz = dout, dlse
    if zero_dout:
        dz = dout * rows[..., None]
        dlz = None if dlse is None else dlse * rows
    if emulate:
        r = _emulate(q, k, v, dz, scale, keep, inv_keep, dlz, valid)
    else:
        r = kr.attn_ref(q, k, v, dz, causal, scale, keep, inv_keep, dlz,
                        valid=valid)
    r = dict(r, dout=dz, dlse_used=dlz)
    if zero_rows:
        r["lse"] = r["lse"] * rows
        for name in ("out", "dq"):
            r[name] = r[name] * rows[..., None]
    return r


class Expected:
    """reference, bounds and criterion of one (inputs, lengths, mask,
    dlse); an empty sample runs as length 1 and is ignored"""

    def __init__(self, inp, lens, d, causal, keep=None, thresh=0,
                 dlse=None):
        q, k, v, dout = inp
        self.seq = q.shape[2]
        self.lens = lens_b1(lens)
        assert int(self.lens.min()) >= 0 and int(self.lens.max()) <= self.seq
        scale = d ** -0.5
        self.ref = model(inp, self.lens.clamp(min=1), causal, scale, keep,
                         kr.attn_inv_keep(thresh), dlse, zero_rows=False)
        # the [B,1,S,S] mask of the issue, as attn_ref took it
        assert self.ref["valid"].shape == (q.shape[0], 1, self.seq, self.seq)
        self.bounds = kr.attn_bounds(self.ref, q, k, v, self.ref["dout"],
                                     scale)

    def ratios(self, got):
        """worst err / E per output.  out, lse, dq: rows < len against the
        reference, rows >= len against exact zero; delta: rows < len only,
        from the kernel's own bf16 out; dk, dv: everywhere (the reference
        is zero on padded rows), all zero for an empty sample."""
        rows = row_mask(self.seq, self.lens)              # [B,1,S]
        alive = (self.lens > 0)[:, :, None]               # [B,1,1]
        res = {}
        for name in kr.ATTN_OUTPUTS:
            want, bound = self.ref[name], self.bounds[name]
            if name == "delta":
                want, bound = kr.attn_delta_ref(
                    self.ref["dout"], got["out"], self.ref["dlse_used"])
            g = got[name]
            sel = alive if name in ("dk", "dv") else rows
            if g.dim() == 4:
                sel = sel[..., None]
            sel = sel.expand(g.shape)
            err = (g - want).abs()
            if name == "delta":
                err = torch.where(sel, err, torch.zeros_like(err))
            else:
                err = torch.where(sel, err, g.abs())
                bound = torch.where(sel, bound, torch.zeros_like(bound))
            res[name] = kr.attn_ratio(err, bound)
        return res
