"""Plain fp64 references and deterministic input builders for the HIP
kernel tests (LAMB phases, sharded cross-entropy, MoE dispatch/combine,
flash attention, LayerNorm, bias + GeLU and the column sum, the last four
with derived per-element rounding bounds).

Everything here runs on the CPU in float64 and is validated without a GPU
by test_kernel_refs_cpu.py; the GPU tests compare the kernels against it.
"""

import math

import torch

F64 = torch.float64


# ---------------------------------------------------------------------------
# LAMB
# ---------------------------------------------------------------------------
def lamb_ref(master, grad, m, v, extents, lr, beta1, beta2, eps,
             weight_decay, step, inv_scale):
    """One LAMB step over a flat arena, FusedLAMB._step_torch's definition.

    master, grad, m, v: fp64 flat tensors (not modified).  extents: list of
    (offset, numel), one per parameter.  Returns a dict with the new m, v,
    the raw update u = mhat / (sqrt(vhat) + eps) + wd * w, the per-parameter
    ||w||^2, ||u||^2 and trust ratio (1 when either norm is 0), and the new
    master w - lr * ratio * u (elements outside every extent: ratio 1).
    """
    assert master.dtype == F64 and grad.dtype == F64
    g = grad * inv_scale
    m_new = beta1 * m + (1.0 - beta1) * g
    v_new = beta2 * v + (1.0 - beta2) * g * g
    mhat = m_new / (1.0 - beta1 ** step)
    vhat = v_new / (1.0 - beta2 ** step)
    update = mhat / (vhat.sqrt() + eps) + weight_decay * master
    wsq = torch.zeros(len(extents), dtype=F64)
    usq = torch.zeros(len(extents), dtype=F64)
    ratio = torch.ones(len(extents), dtype=F64)
    per_elem = torch.ones_like(master)
    for c, (off, n) in enumerate(extents):
        w = master[off:off + n]
        u = update[off:off + n]
        wsq[c] = (w * w).sum()
        usq[c] = (u * u).sum()
        if wsq[c] > 0 and usq[c] > 0:
            ratio[c] = math.sqrt(wsq[c].item()) / max(
                math.sqrt(usq[c].item()), 1e-12)
        per_elem[off:off + n] = ratio[c]
    new_master = master - lr * per_elem * update
    return dict(m=m_new, v=v_new, update=update, wsq=wsq, usq=usq,
                ratio=ratio, master=new_master)


LAMB_SHAPES = [(3,), (130,), (64, 33), (1,), (257,), (4000,)]


def lamb_params(shapes=LAMB_SHAPES, dtype=torch.bfloat16, device="cpu",
                zero_param=1, seed=0):
    """nn.Parameters for a FlatParamGroup.  Parameter ``zero_param`` (index
    into ``shapes``) is all zero; the others are randn.  Magnitudes are
    applied later, per arena chunk, by lamb_fill()."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, s in enumerate(shapes):
        w = torch.randn(*s, generator=gen)
        if i == zero_param:
            w.zero_()
        out.append(torch.nn.Parameter(w.to(dtype).to(device)))
    return out


def lamb_magnitude(chunk):
    return 10.0 ** (chunk % 4)


def lamb_fill(group, seed, grad_mul=1.0, zero_grad_chunk=None,
              scale_weights=False):
    """Write fresh gradients into the group's grad arena: chunk c (the
    group's own arena order) gets randn * 10**(c % 4) * grad_mul; padding
    stays 0.  With scale_weights the weights (param arena and master) are
    multiplied by the same magnitude, once."""
    gen = torch.Generator().manual_seed(seed)
    ga = torch.zeros(group.total, dtype=torch.float32)
    for c, (p, off) in enumerate(zip(group.ordered, group.offsets)):
        n = p.numel()
        if c != zero_grad_chunk:
            ga[off:off + n] = (torch.randn(n, generator=gen) *
                               lamb_magnitude(c) * grad_mul)
        if scale_weights:
            group.param_arena[off:off + n] *= lamb_magnitude(c)
    group.grad_arena.copy_(ga.to(group.grad_arena.dtype))
    if scale_weights:
        group.refresh_master()


def lamb_extents(group):
    return [(off, p.numel()) for p, off in zip(group.ordered, group.offsets)]


def lamb_padded_extents(group):
    """(offset, padded numel) per chunk: the arena range whose chunk_of
    entries must name that chunk."""
    ends = list(group.offsets[1:]) + [group.total]
    return [(off, end - off) for off, end in zip(group.offsets, ends)]


def lamb_padding_mask(group):
    mask = torch.ones(group.total, dtype=torch.bool)
    for off, n in lamb_extents(group):
        mask[off:off + n] = False
    return mask


def lamb_elem_magnitude(group):
    mag = torch.ones(group.total, dtype=F64)
    for c, (off, n) in enumerate(lamb_padded_extents(group)):
        mag[off:off + n] = lamb_magnitude(c)
    return mag


def check_chunk_map(group):
    """The kernels index chunk_of[i >> 3] for EVERY arena element, padding
    included, and use the value as an index into the norm buffers: every
    entry has to be the index of the chunk whose padded extent holds it."""
    cmap = group.state["lamb_chunk_of"].cpu()
    n = group.state["lamb_nchunks"]
    assert cmap.dtype == torch.int32
    assert cmap.numel() == (group.total + 7) // 8
    assert group.total % 8 == 0
    for c, (off, ext) in enumerate(lamb_padded_extents(group)):
        assert off % 8 == 0 and ext % 8 == 0, (off, ext)
        got = cmap[off // 8:(off + ext) // 8]
        assert bool((got == c).all()), (c, got.unique().tolist())
    assert int(cmap.min()) >= 0 and int(cmap.max()) < n


# ---------------------------------------------------------------------------
# Sharded cross-entropy
# ---------------------------------------------------------------------------
def ce_ref(logits, targets, ignore_index, dloss=None, scale=1.0):
    """Per-row loss and dlogits over the FULL vocabulary, in fp64, as
    log_softmax / (softmax - onehot).  Ignored rows: loss 0, gradient 0."""
    lf = logits.to(F64)
    rows = lf.shape[0]
    logp = torch.log_softmax(lf, dim=1)
    valid = targets != ignore_index
    safe = torch.where(valid, targets, torch.zeros_like(targets))
    loss = -logp.gather(1, safe[:, None]).squeeze(1)
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    if dloss is None:
        dloss = torch.ones(rows, dtype=F64)
    onehot = torch.zeros_like(lf)
    onehot[torch.arange(rows), safe] = 1.0
    dl = torch.where(valid, dloss.to(F64) * scale, torch.zeros(rows, dtype=F64))
    dlogits = (torch.softmax(lf, dim=1) - onehot) * dl[:, None]
    return loss, dlogits


def ce_shard_stats_ref(shard, targets, vocab_begin, ignore_index):
    """fp64 row max, sum exp(x - max) and target logit of one shard."""
    sf = shard.to(F64)
    cols = sf.shape[1]
    rmax = sf.max(dim=1).values
    rsum = torch.exp(sf - rmax[:, None]).sum(dim=1)
    inside = ((targets != ignore_index) & (targets >= vocab_begin) &
              (targets < vocab_begin + cols))
    safe = (targets - vocab_begin).clamp(0, cols - 1)
    tl = torch.where(inside, sf.gather(1, safe[:, None]).squeeze(1),
                     torch.zeros(sf.shape[0], dtype=F64))
    return rmax, rsum, tl


CE_HOT = 1          # row with logits around +100
CE_GAP60 = 2        # row whose max is 60 above every other shard
CE_EQUAL = 3        # row with all logits equal
CE_GAP120 = 4       # as CE_GAP60 with a gap whose exp is 0 in fp32
CE_PEAK_COL = 3     # column (shard 0) holding the peak of the gap rows


def ce_required_targets(widths):
    """For every shard boundary b: b - 1 and b; the last column; class 0."""
    vocab = sum(widths)
    req = []
    b = 0
    for w in widths[:-1]:
        b += w
        req += [b, b - 1]
    req += [vocab - 1, 0]
    return req


def ce_case(rows, widths, dtype, ignore_index=-100, seed=0):
    """Deterministic logits / targets / dloss for the sharded CE tests.

    logits: [rows, sum(widths)] in ``dtype``, uniform in (-8, 8) except
    the constructed rows (present when rows > their index; the gap rows
    only with more than one shard).  targets: rows 0.. take the required
    targets in turn, the rest are spread over the vocabulary; every 7th
    row (6, 13, ...) is ignored.  dloss: non-uniform, in [0.5, 1.5).
    """
    vocab = sum(widths)
    gen = torch.Generator().manual_seed(seed)
    logits = (torch.rand(rows, vocab, generator=gen, dtype=F64) * 16 - 8)
    special = {}
    if rows > CE_HOT:
        logits[CE_HOT] = 100 + logits[CE_HOT] / 2
        special["hot"] = CE_HOT
    if len(widths) > 1:
        if rows > CE_GAP60:
            logits[CE_GAP60, CE_PEAK_COL] = \
                logits[CE_GAP60, widths[0]:].max() + 60
            special["gap60"] = CE_GAP60
        if rows > CE_GAP120:
            logits[CE_GAP120, CE_PEAK_COL] = \
                logits[CE_GAP120, widths[0]:].max() + 120
            special["gap120"] = CE_GAP120
    if rows > CE_EQUAL:
        logits[CE_EQUAL] = 1.5
        special["equal"] = CE_EQUAL
    logits = logits.to(dtype)

    req = ce_required_targets(widths)
    targets = torch.empty(rows, dtype=torch.long)
    for r in range(rows):
        if r < len(req):
            targets[r] = req[r]
        else:
            targets[r] = (r * 2654435761 + 12345) % vocab
    # a run of required targets that an ignored row interrupts continues
    # after it, so every required target is on a live row when rows allow
    live = [r for r in range(rows) if r % 7 != 6]
    for r, t in zip(live, req):
        targets[r] = t
    targets[6::7] = ignore_index
    dloss = 0.5 + torch.rand(rows, generator=gen, dtype=F64)
    return logits, targets, dloss.float(), special


# ---------------------------------------------------------------------------
# MoE dispatch / combine
# ---------------------------------------------------------------------------
def moe_assignment_from_topi(topi, num_experts):
    """ExpertParallelMLP.forward's slot assignment: stable argsort by
    expert, segmented arange, inv[order] = arange.  Returns fe, pos, ft,
    inv, order."""
    n_tokens, k = topi.shape
    flat_e = topi.reshape(-1)
    flat_t = torch.arange(n_tokens).repeat_interleave(k)
    order = torch.argsort(flat_e, stable=True)
    fe, ft = flat_e[order], flat_t[order]
    counts = torch.zeros(num_experts, dtype=torch.long)
    counts.scatter_add_(0, fe, torch.ones_like(fe))
    seg_start = torch.nn.functional.pad(counts.cumsum(0), (1, 0))[:-1]
    pos = torch.arange(fe.numel()) - seg_start[fe]
    inv = torch.empty_like(order)
    inv[order] = torch.arange(fe.numel())
    return (fe.contiguous(), pos.contiguous(), ft.contiguous(),
            inv.contiguous(), order)


def moe_topi(n_tokens, k, num_experts, pattern):
    t = torch.arange(n_tokens)
    if pattern == "skew":
        # first choice always expert 0, second cycles over 1 and 2, the
        # last expert receives nothing
        assert k == 2 and num_experts >= 4
        return torch.stack([torch.zeros_like(t), 1 + t % 2], dim=1)
    if pattern == "cyclic":
        return torch.stack([(t + j) % num_experts for j in range(k)], dim=1)
    if pattern == "uneven1":
        # k = 1: every third token to expert 0, the rest spread unevenly
        assert k == 1
        e = torch.where(t % 3 == 0, torch.zeros_like(t),
                        (t // 2) % num_experts)
        return e[:, None]
    raise ValueError(pattern)


def moe_assignment(n_tokens, k, num_experts, cap, pattern):
    """Deterministic assignment lists fe, pos, ft, inv (int64) and fw
    (fp32, distinct per assignment, in (0.1, 0.9)), in the expert-sorted
    order the kernels take.  ``cap`` does not change the lists (the
    kernels skip pos >= cap themselves); it is checked for sanity only."""
    assert cap >= 1
    topi = moe_topi(n_tokens, k, num_experts, pattern)
    fe, pos, ft, inv, order = moe_assignment_from_topi(topi, num_experts)
    m = n_tokens * k
    # distinct weights in token-major order, scrambled so neighbours differ
    idx = (torch.arange(m) * 7919) % m if math.gcd(7919, m) == 1 \
        else torch.arange(m)
    flat_w = (0.1 + 0.8 * (idx.to(F64) + 0.5) / m).float()
    fw = flat_w[order].contiguous()
    return fe, pos, ft, inv, fw


def moe_properties(fe, pos, ft, k, num_experts, cap, n_tokens):
    keep = pos < cap
    kept_per_token = torch.zeros(n_tokens, dtype=torch.long)
    kept_per_token.scatter_add_(0, ft, keep.long())
    per_expert = torch.zeros(num_experts, dtype=torch.long)
    per_expert.scatter_add_(0, fe, torch.ones_like(fe))
    return dict(
        dropped=int((~keep).sum()),
        half_kept=bool(((kept_per_token > 0) & (kept_per_token < k)).any()),
        none_kept=bool((kept_per_token == 0).any()),
        empty_expert=bool((per_expert == 0).any()),
        kept_per_token=kept_per_token,
    )


def moe_check_lists(fe, pos, ft, inv, k, num_experts, n_tokens):
    """Everything the kernels index with, checked against the buffer
    extents before a launch."""
    m = n_tokens * k
    for t in (fe, pos, ft, inv):
        assert t.dtype == torch.long and t.numel() == m
    assert int(fe.min()) >= 0 and int(fe.max()) < num_experts
    assert int(ft.min()) >= 0 and int(ft.max()) < n_tokens
    assert int(pos.min()) >= 0
    assert torch.equal(torch.sort(inv).values, torch.arange(m))
    # token t's k assignments are inv[t*k : t*k+k]
    assert torch.equal(ft[inv], torch.arange(n_tokens).repeat_interleave(k))
    # (expert, pos) pairs are unique: every write goes to its own row
    key = fe * (int(pos.max()) + 1) + pos
    assert key.unique().numel() == m


# (pattern, k, cap) at n_tokens = 96, 4 experts, and what each is for
MOE_PATTERNS = {
    "skew": ("skew", 2, 48),
    "all_dropped": ("skew", 2, 10),
    "roomy": ("cyclic", 2, 192),
    "top1": ("uneven1", 1, 20),
    "cap1": ("skew", 2, 1),
}
MOE_CLAIMS = {
    "skew": dict(dropped=True, half_kept=True, none_kept=False,
                 empty_expert=True),
    "all_dropped": dict(dropped=True, half_kept=True, none_kept=True,
                        empty_expert=True),
    "roomy": dict(dropped=False, half_kept=False, none_kept=False,
                  empty_expert=False),
    "top1": dict(dropped=True, half_kept=False, none_kept=True,
                 empty_expert=False),
    "cap1": dict(dropped=True, half_kept=True, none_kept=True,
                 empty_expert=True),
}


def moe_check_claims(name, fe, pos, ft, inv, k, num_experts, cap, n_tokens):
    moe_check_lists(fe, pos, ft, inv, k, num_experts, n_tokens)
    props = moe_properties(fe, pos, ft, k, num_experts, cap, n_tokens)
    claims = MOE_CLAIMS[name]
    assert (props["dropped"] > 0) == claims["dropped"], props
    for key in ("half_kept", "none_kept", "empty_expert"):
        assert props[key] == claims[key], (name, key, props)
    return props


def moe_dispatch_fwd_ref(x, fe, pos, ft, num_experts, cap):
    """disp[fe, pos] = x[ft] for kept assignments.  Returns (disp fp64
    [E, cap, H], written [E, cap] bool)."""
    keep = pos < cap
    disp = torch.zeros(num_experts, cap, x.shape[-1], dtype=F64)
    written = torch.zeros(num_experts, cap, dtype=torch.bool)
    disp[fe[keep], pos[keep]] = x.to(F64)[ft[keep]]
    written[fe[keep], pos[keep]] = True
    return disp, written


def moe_dispatch_bwd_ref(ddisp, fe, pos, ft, n_tokens, cap):
    keep = pos < cap
    dx = torch.zeros(n_tokens, ddisp.shape[-1], dtype=F64)
    dx.index_add_(0, ft[keep], ddisp.to(F64)[fe[keep], pos[keep]])
    return dx


def moe_combine_fwd_ref(h, fw, fe, pos, ft, n_tokens, cap):
    """out[t] = sum over t's kept assignments of fw * h[fe, pos].  Also
    returns sum |fw * h| for the error bound."""
    keep = pos < cap
    terms = h.to(F64)[fe[keep], pos[keep]] * fw.to(F64)[keep][:, None]
    out = torch.zeros(n_tokens, h.shape[-1], dtype=F64)
    mag = torch.zeros_like(out)
    out.index_add_(0, ft[keep], terms)
    mag.index_add_(0, ft[keep], terms.abs())
    return out, mag


def moe_combine_bwd_ref(dout, h, fw, fe, pos, ft, num_experts, cap):
    """dh[fe, pos] = fw * dout[ft] (kept), dfw = <dout[ft], h[fe, pos]>
    (0 for dropped).  Also returns sum |dout * h| per assignment."""
    keep = pos < cap
    d = dout.to(F64)[ft[keep]]
    hk = h.to(F64)[fe[keep], pos[keep]]
    dh = torch.zeros(num_experts, cap, h.shape[-1], dtype=F64)
    dh[fe[keep], pos[keep]] = d * fw.to(F64)[keep][:, None]
    dfw = torch.zeros(fe.numel(), dtype=F64)
    mag = torch.zeros(fe.numel(), dtype=F64)
    dfw[keep] = (d * hk).sum(dim=1)
    mag[keep] = (d * hk).abs().sum(dim=1)
    return dh, dfw, mag


# ---------------------------------------------------------------------------
# Flash attention
# ---------------------------------------------------------------------------
ATTN_B, ATTN_H = 2, 3      # b != h, so bh / heads vs bh % heads shows
U_BF16 = 2.0 ** -8          # bf16 unit roundoff used by attn_bounds
ATTN_SENTINEL16 = 0x7FA5    # a bf16 NaN: a stray read poisons the result
ATTN_SENTINEL32 = 0x7FA55AA5  # an fp32 NaN
ATTN_FAMILIES = ("randn", "peaked", "shifted")
ATTN_LAYOUTS = ("plain", "qkv", "padded")
ATTN_PEAK_KEYS = (0, 31, 32, 63, 64, 127, 128)
# the GPU matrix (test_attention_fp64_gpu.py); test_kernel_refs_cpu.py
# proves the bounds on the same cases
ATTN_DIMS = (64, 128)
ATTN_SEQS = (1, 31, 32, 33, 64, 65, 72, 127, 128, 129, 200, 257)
ATTN_CROSSED_SEQS = (72, 200)     # every layout
ATTN_DROP_SEQS = (33, 72, 200, 257)
ATTN_DROP_FAMILY = {1: "randn", 128: "peaked", 255: "shifted"}
ATTN_DLSE_SEQS = (72, 200)
ATTN_COMBINED_SEQS = (33, 64, 72, 200, 257)
ATTN_ENV_SEQS = (72, 200, 257)
ATTN_OUTPUTS = ("out", "lse", "delta", "dq", "dk", "dv")
# allowed err / E: the derived bound is proven at 1 x E for the rounding
# model on the CPU; the kernels get twice that on the bf16 outputs
ATTN_FACTOR = dict(out=2.0, lse=1.0, delta=1.0, dq=2.0, dk=2.0, dv=2.0)


def attn_env_cases(dbuf):
    """(d, seq, causal, thresh, family) run by the child process of one
    EPL_ATTN_BWD_DBUF setting: d128 always stages directly, so it runs in
    the dbuf-0 children only; the families rotate"""
    dims = ATTN_DIMS if dbuf == 0 else (64,)
    cases = [(d, seq, causal, thresh)
             for d in dims for seq in ATTN_ENV_SEQS
             for causal in (False, True) for thresh in (0, 128)]
    return [c + (ATTN_FAMILIES[i % len(ATTN_FAMILIES)],)
            for i, c in enumerate(cases)]


def attn_inv_keep(thresh):
    return 256.0 / (256 - thresh)


def attn_ratio(err, bound):
    """worst err / bound over the elements; 0 / 0 counts as 0 and a
    non-zero error at a zero bound as inf"""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if bool(torch.isfinite(err).all()) else \
        float("inf")


def bf16_round(x):
    """fp64 -> nearest bf16 (ties to even) -> fp64"""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def attn_valid(sq, sk, causal):
    valid = torch.ones(sq, sk, dtype=torch.bool)
    return torch.tril(valid) if causal else valid


def attn_ref(q, k, v, dout, causal, scale, keep=None, inv_keep=1.0,
             dlse=None, valid=None):
    """Softmax attention forward and backward by explicit fp64 formulas
    (no autograd).  q, dout: [B,H,Sq,D]; k, v: [B,H,Sk,D]; keep: [B,H,Sq,Sk]
    0/1 dropout keep bits or None; dlse: [B,H,Sq] cotangent of lse or None;
    valid: [Sq,Sk] bool key mask overriding ``causal`` (used by the mutation
    tests).  delta follows the dQ kernel: rowsum(dout o out) - dlse."""
    assert q.dtype == F64 and k.dtype == F64 and v.dtype == F64
    if valid is None:
        valid = attn_valid(q.shape[-2], k.shape[-2], causal)
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    sm = s.masked_fill(~valid, float("-inf"))
    mx = sm.max(dim=-1, keepdim=True).values
    e = torch.exp(sm - mx)
    l = e.sum(dim=-1, keepdim=True)
    lse = (mx + l.log()).squeeze(-1)
    p = e / l
    pd = p if keep is None else p * keep * inv_keep
    out = torch.matmul(pd, v)
    dl = torch.zeros_like(lse) if dlse is None else dlse
    delta = (dout * out).sum(dim=-1) - dl
    dp = torch.matmul(dout, v.transpose(-1, -2))
    if keep is not None:
        dp = dp * keep * inv_keep
    ds = p * (dp - delta.unsqueeze(-1)) * scale
    return dict(s=s, lse=lse, P=p, Pd=pd, out=out, delta=delta, dP=dp,
                dS=ds, dq=torch.matmul(ds, k),
                dk=torch.matmul(ds.transpose(-1, -2), q),
                dv=torch.matmul(pd.transpose(-1, -2), dout),
                dlse=dl, valid=valid)


def attn_delta_ref(dout, out_used, dlse=None):
    """delta = rowsum(dout o out_used) - dlse in fp64 and its bound: the
    kernel sums the d products of the bf16 ``out_used`` it reads in fp32."""
    prod = dout * out_used
    dl = torch.zeros(prod.shape[:-1], dtype=F64) if dlse is None else dlse
    return (prod.sum(dim=-1) - dl,
            2.0 ** -16 * (prod.abs().sum(dim=-1) + dl.abs()))


def attn_bounds(ref, q, k, v, dout, scale):
    """Per-element rounding bounds of the kernels' results against
    attn_ref, u = 2^-8.  The kernels round P once (operand of the PV and dV
    MFMAs), round dS once, round every stored output once and take delta
    from the bf16 out; everything else is fp32.

    out  : u (Pd |V|) + u |out|
    dv   : u (Pd^T |dout|) + u |dv|
    dS   : scale P (u rowsum(|dout| o |out|)) + u |dS|   (delta, then dS)
    dq   : E_dS |K| + u |dq|;  dk : E_dS^T |Q| + u |dk|
    lse  : 2^-16 (1 + max_j A_ij), A = scale |Q| |K|^T: a d-term fp32
           dot product is off by at most d 2^-24 A (d <= 128), the rest is
           the argument rounding of __expf / __logf, with margin
    delta: see attn_delta_ref
    """
    u = U_BF16
    p, pd = ref["P"], ref["Pd"]
    e_out = u * torch.matmul(pd, v.abs()) + u * ref["out"].abs()
    e_dv = (u * torch.matmul(pd.transpose(-1, -2), dout.abs()) +
            u * ref["dv"].abs())
    rs = (dout.abs() * ref["out"].abs()).sum(dim=-1, keepdim=True)
    e_ds = scale * p * (u * rs) + u * ref["dS"].abs()
    e_dq = torch.matmul(e_ds, k.abs()) + u * ref["dq"].abs()
    e_dk = torch.matmul(e_ds.transpose(-1, -2), q.abs()) + u * ref["dk"].abs()
    a = scale * torch.matmul(q.abs(), k.abs().transpose(-1, -2))
    a = a.masked_fill(~ref["valid"], 0.0)
    e_lse = 2.0 ** -16 * (1.0 + a.max(dim=-1).values)
    _, e_delta = attn_delta_ref(dout, ref["out"], ref["dlse"])
    return dict(out=e_out, lse=e_lse, delta=e_delta, dq=e_dq, dk=e_dk,
                dv=e_dv)


def attn_emulate(q, k, v, dout, causal, scale, keep=None, inv_keep=1.0,
                 dlse=None):
    """attn_ref's arithmetic with the kernels' bf16 roundings inserted:
    the forward rounds exp(s - max) * keep * inv_keep before the PV product
    and normalises after it, the backward rounds P * keep * inv_keep (dV)
    and dS, every stored output is rounded, delta comes from the rounded
    out.  delta_from is that out, for attn_delta_ref."""
    valid = attn_valid(q.shape[-2], k.shape[-2], causal)
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    sm = s.masked_fill(~valid, float("-inf"))
    mx = sm.max(dim=-1, keepdim=True).values
    e = torch.exp(sm - mx)
    l = e.sum(dim=-1, keepdim=True)
    lse = (mx + l.log()).squeeze(-1)
    kf = 1.0 if keep is None else keep * inv_keep
    out = bf16_round(torch.matmul(bf16_round(e * kf), v) / l)
    dl = torch.zeros_like(lse) if dlse is None else dlse
    delta = (dout * out).sum(dim=-1) - dl
    p = torch.exp(sm - lse.unsqueeze(-1))
    pd = bf16_round(p * kf)
    dp = torch.matmul(dout, v.transpose(-1, -2)) * kf
    ds = bf16_round(p * (dp - delta.unsqueeze(-1)) * scale)
    return dict(out=out, lse=lse, delta=delta, delta_from=out,
                dq=bf16_round(torch.matmul(ds, k)),
                dk=bf16_round(torch.matmul(ds.transpose(-1, -2), q)),
                dv=bf16_round(torch.matmul(pd.transpose(-1, -2), dout)))


def attn_peak_pairs(seq, causal):
    """(query row, dominating key) pairs of the ``peaked`` family: every
    key of ATTN_PEAK_KEYS below seq and key seq-1, each on a row of its
    own (at or below the diagonal when causal); causal adds rows peaked on
    their diagonal and on the key before it."""
    keys = [j for j in ATTN_PEAK_KEYS if j < seq - 1] + [seq - 1]
    pairs, used = [], set()

    def place(row_candidates, key):
        for r in row_candidates:
            if 0 <= r < seq and r not in used and (not causal or r >= key):
                used.add(r)
                pairs.append((r, key))
                return

    for t, j in enumerate(reversed(keys)):
        # key seq-1 first (causal: only row seq-1 sees it), then rows
        # spread downwards over the sequence
        place(list(range(seq - 1 - 3 * t, -1, -1)) +
              list(range(seq - 1, -1, -1)), j)
    if causal:
        for r in (seq // 2, seq // 3, 1):
            place([r], r)
        for r in (seq // 2 + 1, seq // 3 + 1, 2):
            if r >= 1:
                place([r], r - 1)
    return pairs


def attn_inputs(family, seq, d, causal=False, seed=0, b=ATTN_B, h=ATTN_H):
    """q, k, v, dout: fp64 [b,h,seq,d] holding bf16-representable values,
    from a seeded generator.

    randn   : standard normal.
    peaked  : q, k scaled so max |s| is about 40 (single keys dominate
              rows), plus the steered rows of attn_peak_pairs with
              s = 40 on the chosen key.
    shifted : a unit direction w added as +-c w to q rows (sign by row)
              and +c w to k, c^2 scale = 60: every score of a row carries a
              common offset of about +-60, differences stay O(1).
    """
    assert family in ATTN_FAMILIES
    gen = torch.Generator().manual_seed(
        seed + 1000 * ATTN_FAMILIES.index(family) + 7 * seq + d +
        (500 if causal else 0))
    scale = 1.0 / math.sqrt(d)
    q, k, v, dout = (torch.randn(b, h, seq, d, generator=gen, dtype=F64)
                     for _ in range(4))
    if family == "peaked":
        smax = (torch.matmul(q, k.transpose(-1, -2)) * scale).abs().max()
        f = math.sqrt(40.0 / smax.item())
        q, k = q * f, bf16_round(k * f)
        for row, key in attn_peak_pairs(seq, causal):
            kj = k[:, :, key]
            q[:, :, row] = kj * (40.0 / (scale * (kj * kj).sum(
                dim=-1, keepdim=True)))
    elif family == "shifted":
        w = torch.randn(b, h, 1, d, generator=gen, dtype=F64)
        w = w / w.norm(dim=-1, keepdim=True)
        c = math.sqrt(60.0 / scale)
        sign = torch.where((torch.arange(seq) // 2) % 2 == 0, 1.0, -1.0)
        q = q + c * sign.to(F64)[None, None, :, None] * w
        k = k + c * w
    return bf16_round(q), bf16_round(k), bf16_round(v), bf16_round(dout)


def attn_dlse(seq, seed=0, b=ATTN_B, h=ATTN_H):
    """a non-zero cotangent of lse, fp32-representable, fp64 [b,h,seq]"""
    gen = torch.Generator().manual_seed(4242 + seed + seq)
    return torch.randn(b, h, seq, generator=gen).to(F64)


def unpack_keep(mask_words, bh, seq):
    """keep bits [bh, seq, seq] (fp64 0/1) from the forward's published
    int32 mask words [bh * seq * ceil(seq/32)]: bit kv & 31 of word
    kv >> 5 of row q"""
    words = mask_words.reshape(bh, seq, (seq + 31) // 32).to(torch.int64)
    shifts = torch.arange(32, device=words.device)
    bits = ((words.unsqueeze(-1) >> shifts) & 1).reshape(bh, seq, -1)
    return bits[:, :, :seq].to(F64)


class GuardedBuffer:
    """A flat device buffer pre-filled with a sentinel bit pattern, a
    strided view into it behind ``guard`` leading elements, and the map of
    the elements that view addresses."""

    def __init__(self, shape, strides, offset, dtype, device, guard):
        sentinel, idt = {
            2: (ATTN_SENTINEL16, torch.int16),
            4: (ATTN_SENTINEL32, torch.int32)}[dtype.itemsize]
        if sentinel >= 2 ** (8 * dtype.itemsize - 1):
            sentinel -= 2 ** (8 * dtype.itemsize)
        offset += guard
        extent = offset + 1 + sum(
            (n - 1) * st for n, st in zip(shape, strides))
        self.sentinel = sentinel
        self.raw = torch.full((extent + guard,), sentinel, dtype=idt,
                              device=device)
        self.view = self.raw.view(dtype).as_strided(shape, strides, offset)
        self.addressed = torch.zeros(extent + guard, dtype=torch.bool)
        self.addressed.as_strided(shape, strides, offset).fill_(True)

        self.guard = guard

    def sub(self, shape, strides, offset):
        """a strided view of addressed elements only (the qkv slices)"""
        offset += self.guard
        assert bool(self.addressed.as_strided(shape, strides, offset).all())
        return self.raw.view(self.view.dtype).as_strided(
            shape, strides, offset)

    def stray_writes(self):
        """number of unaddressed elements that lost the sentinel"""
        raw = self.raw.cpu()
        return int(((raw != self.sentinel) & ~self.addressed).sum())


def attn_flat(n, dtype, device, guard=64):
    """guarded contiguous [n] buffer (lse, delta, mask words)"""
    return GuardedBuffer((n,), (1,), 0, dtype, device, guard)


def attn_layout(name, b, h, seq, d, device, dtype=torch.bfloat16):
    """Views q, k, v, out, dout, dq, dk, dv (all [b,h,seq,d]) and their
    GuardedBuffers (``buffers``: name -> buffer), every element pre-filled
    with the sentinel and two rows of guard on either side.

    plain : q/k/v/dout/grads contiguous [b,h,seq,d]; out in [b,seq,h,d]
            memory order.
    qkv   : q/k/v slices of one [b,seq,3,h,d] buffer, the gradients slices
            of one d_qkv buffer, out and dout in [b,seq,h,d] order.
    padded: inputs with row stride d+8 at storage offset 8, out
            contiguous [b,h,seq,d], dout a permuted [b,seq,h,d] view, the
            gradients with row stride d+16 at storage offset 16: the four
            stride triplets differ.
    """
    shape = (b, h, seq, d)
    guard = 2 * (d + 16)
    bhsd = (h * seq * d, seq * d, d, 1)
    bshd = (seq * h * d, d, h * d, 1)
    bufs, views = {}, {}

    def own(key, strides, offset=0):
        bufs[key] = GuardedBuffer(shape, strides, offset, dtype, device,
                                  guard)
        views[key] = bufs[key].view

    if name == "plain":
        for key in ("q", "k", "v", "dout", "dq", "dk", "dv"):
            own(key, bhsd)
        own("out", bshd)
    elif name == "qkv":
        packed = (seq * 3 * h * d, d, 3 * h * d, 1)
        for buf_key, keys in (("qkv", ("q", "k", "v")),
                              ("d_qkv", ("dq", "dk", "dv"))):
            bufs[buf_key] = GuardedBuffer(
                (b, seq, 3, h, d),
                (seq * 3 * h * d, 3 * h * d, h * d, d, 1), 0, dtype,
                device, guard)
            for i, key in enumerate(keys):
                views[key] = bufs[buf_key].sub(shape, packed, i * h * d)
        own("out", bshd)
        own("dout", bshd)
    elif name == "padded":
        pin = (h * seq * (d + 8), seq * (d + 8), d + 8, 1)
        pg = (h * seq * (d + 16), seq * (d + 16), d + 16, 1)
        for key in ("q", "k", "v"):
            own(key, pin, 8)
        for key in ("dq", "dk", "dv"):
            own(key, pg, 16)
        own("out", bhsd)
        own("dout", bshd)
    else:
        raise ValueError(name)
    views["buffers"] = bufs
    return views


# ---------------------------------------------------------------------------
# LayerNorm, bias + GeLU, column sum
# ---------------------------------------------------------------------------
U_F32 = 2.0 ** -24          # fp32 unit roundoff
V_BF16 = 2.0 ** -9          # one bf16 round-to-nearest: |fl(a) - a| <= 2^-9 |a|
TINY_F32 = 2.0 ** -126      # below this fp32 flushes or loses bits
LN_EPS = 1e-5
# the rstd bound has to stay below this on every row of the matrix, so
# that rstd never sets the bound of out (half a bf16 rounding is 2^-9)
LN_RSTD_REL_MAX = 2.0 ** -12


def f32_round(x):
    return x.to(torch.float32).to(F64)


def gamma_k(k):
    """k fp32 roundings in sequence: (1 + u)^k - 1 <= k u / (1 - k u)"""
    return k * U_F32 / (1.0 - k * U_F32)


def ratio_of(got, want, bound):
    return attn_ratio((got - want).abs(), bound)


# ---- input families -------------------------------------------------------
# kind -> (family, parameters).  near_const: (base, elements one bf16 step
# up); the step is the bf16 spacing at the base.
LN_KINDS = (
    ("randn", "randn", None),
    ("off16", "offset", (1.0, 16.0)),
    ("off300", "offset", (1.0, 300.0)),
    ("off1000", "offset", (4.0, 1000.0)),
    ("nc100", "near_const", (100.0, 0.5, 3)),
    ("nc128", "near_const", (128.0, 1.0, 2)),
    ("nc250", "near_const", (250.0, 1.0, 9)),
    ("nc1000", "near_const", (1000.0, 4.0, 5)),
    ("const0", "const", 0.0),
    ("const3", "const", 3.3),
    ("const100", "const", 100.5),
    ("tiny", "tiny", None),
    ("one_hot", "one_hot", None),
)
LN_FAMILIES = ("randn", "offset", "near_const", "const", "tiny", "one_hot")
LN_DY_FAMILIES = ("coherent", "cancel")


def ln_row_kinds(rows, rot=0):
    """index into LN_KINDS of every row: the kinds in turn, from ``rot``"""
    return (torch.arange(rows) + rot) % len(LN_KINDS)


def dy_family(name, rows, cols, gen):
    """Upstream gradients for the column sums, bf16-representable fp64.
    coherent: one sign down each column, so |sum| = sum |addend| and the
    bound is a relative one.  cancel: rows in pairs (r, r+1) with opposite
    dy, so the column sum of dy is 0 (the last row of an odd count stays)
    while sum |addend| is as large: the bound is an absolute one."""
    dy = bf16_round(torch.randn(rows, cols, generator=gen, dtype=F64))
    if name == "coherent":
        sign = torch.where(torch.arange(cols) % 3 == 0, -1.0, 1.0).to(F64)
        return dy.abs() * sign
    assert name == "cancel"
    half = rows // 2
    dy[1:2 * half:2] = -dy[0:2 * half:2]
    return dy


def ln_inputs(rows, cols, with_res, dy_name="coherent", rot=0, seed=0):
    """LayerNorm inputs as fp64 tensors of bf16-representable values.

    Row r is of kind LN_KINDS[(r + rot) % 13].  Without a residual x is
    the constructed row.  With one, the constructed row is the sum s and
    res is a few bf16 steps of s per element, x = s - res where that is
    representable (res = 0 elsewhere), so x + res is s exactly; the randn
    kind takes independent randn x and res, whose sum is not representable
    and exercises the rounding of s.  gamma, beta: randn with a zero
    column (cols // 3) and a negative one (the last)."""
    gen = torch.Generator().manual_seed(
        seed + 31 * rows + 1009 * cols + (7 if with_res else 0) + 13 * rot)
    kinds = ln_row_kinds(rows, rot)
    z = torch.randn(rows, cols, generator=gen, dtype=F64)
    s = z.clone()
    for k, (_, family, par) in enumerate(LN_KINDS):
        idx = (kinds == k).nonzero().squeeze(1)
        if idx.numel() == 0 or family == "randn":
            continue
        if family == "offset":
            s[idx] = z[idx] * par[0] + par[1]
        elif family == "near_const":
            base, step, m = par
            m = max(1, min(m, cols // 2))
            pos = torch.rand(idx.numel(), cols, generator=gen).argsort(1)
            row = torch.full((idx.numel(), cols), base, dtype=F64)
            row.scatter_(1, pos[:, :m], base + step)
            s[idx] = row
        elif family == "const":
            s[idx] = par
        elif family == "tiny":
            s[idx] = z[idx] * 2.0 ** -20
        elif family == "one_hot":
            hot = torch.randint(0, cols, (idx.numel(),), generator=gen)
            row = torch.zeros(idx.numel(), cols, dtype=F64)
            row[torch.arange(idx.numel()), hot] = 1000.0
            s[idx] = row
    s = bf16_round(s)
    res = None
    x = s
    if with_res:
        _, e = torch.frexp(s)
        ulp = torch.where(s == 0, torch.full_like(s, 0.125),
                          torch.pow(2.0, (e - 8).to(F64)))
        steps = torch.randint(-3, 4, (rows, cols), generator=gen).to(F64)
        res = steps * ulp
        x = s - res
        bad = (bf16_round(x) != x) | (bf16_round(res) != res)
        res = torch.where(bad, torch.zeros_like(res), res)
        x = torch.where(bad, s, x)
        plain = (kinds == 0).nonzero().squeeze(1)
        if plain.numel():
            res[plain] = bf16_round(torch.randn(
                plain.numel(), cols, generator=gen, dtype=F64))
            x[plain] = s[plain]
    gamma = bf16_round(torch.randn(cols, generator=gen, dtype=F64))
    beta = bf16_round(torch.randn(cols, generator=gen, dtype=F64))
    gamma[cols // 3] = 0.0
    beta[cols // 3] = 0.0
    gamma[cols - 1] = -1.5
    beta[cols - 1] = -0.75
    dy = dy_family(dy_name, rows, cols, gen)
    dadd = bf16_round(torch.randn(rows, cols, generator=gen, dtype=F64))
    return dict(x=x, res=res, gamma=gamma, beta=beta, dy=dy, dadd=dadd,
                kinds=kinds)


# ---- the launch paths, as counts read from csrc/kernels/kernels.hip ---------
def ln_fwd_path(cols, bf16):
    """fast: layer_norm_fwd_bf16_kernel (block from ln_block_for, one or
    two 8-column chunks per thread); else layer_norm_fwd_kernel (256
    threads striding the row).  depth = additions on the longest path of a
    row sum: the thread's own addends, six shuffle steps, two more across
    the (at most four) waves."""
    if bf16 and cols % 8 == 0 and cols <= 4096:
        need = (cols + 7) // 8
        block = 64 if need <= 64 else 128 if need <= 128 else \
            192 if need <= 192 else 256
        chunks = 2 if cols > block * 8 else 1
        return dict(fast=True, block=block, chunks=chunks,
                    depth=8 * chunks + 8)
    return dict(fast=False, block=256, chunks=None,
                depth=(cols + 255) // 256 + 8)


def ln_bwd_path(cols, bf16):
    """fast: layer_norm_bwd_bf16_kernel, one row per wave, CHUNKS 1 / 2 / 4
    chunks of 8 columns per lane and six shuffle steps; else
    layer_norm_bwd_kernel with a 256-thread block per row."""
    if bf16 and cols % 8 == 0 and cols <= 2048:
        chunks = 1 if cols <= 512 else 2 if cols <= 1024 else 4
        return dict(fast=True, chunks=chunks, depth=8 * chunks + 6)
    return dict(fast=False, chunks=None, depth=(cols + 255) // 256 + 8)


def ln_bwd_waves(rows):
    """partial rows (= waves) of the fast backward: ln_bwd_fast_launch"""
    return min((rows + 3) // 4, 1024) * 4


# ---- references --------------------------------------------------------------
def ln_ref(x, res, gamma, beta, eps=LN_EPS):
    """LayerNorm forward in fp64: statistics of the exact s = x + res."""
    s = x if res is None else x + res
    mean = s.mean(dim=1)
    d = s - mean[:, None]
    var = (d * d).mean(dim=1)
    rstd = (var + eps) ** -0.5
    xhat = d * rstd[:, None]
    return dict(s=s, mean=mean, var=var, rstd=rstd, xhat=xhat,
                out=xhat * gamma + beta)


def ln_bwd_ref(dy, x, gamma, mean, rstd, dadd=None):
    """LayerNorm backward in fp64 at the x / mean / rstd the kernel is
    handed: dx = (dyg - (sum dyg + xhat sum dyg xhat) / n) rstd (+ dadd),
    dgamma = sum_rows dy xhat, dbeta = sum_rows dy, colsum = sum_rows dx
    (before any rounding of dx)."""
    n = x.shape[1]
    xhat = (x - mean[:, None]) * rstd[:, None]
    dyg = dy * gamma
    a = dyg.sum(dim=1, keepdim=True)
    b = (dyg * xhat).sum(dim=1, keepdim=True)
    dx_ln = (dyg - (a + xhat * b) / n) * rstd[:, None]
    dx = dx_ln if dadd is None else dx_ln + dadd
    return dict(xhat=xhat, dyg=dyg, a=a, b=b, dx_ln=dx_ln, dx=dx,
                dgamma=(dy * xhat).sum(dim=0), dbeta=dy.sum(dim=0),
                colsum=dx.sum(dim=0))


def colsum_ref(dy):
    return dy.sum(dim=0)


# ---- bounds ------------------------------------------------------------------
def ln_fwd_bounds(ref, x, res, gamma, beta, bf16, eps=LN_EPS):
    """Per-element bounds of the forward kernels against ln_ref.
    u = 2^-24, v = 2^-9, n = cols, k = path depth (ln_fwd_path).

    s    : the kernel forms s32 = fl32(x + res), one IEEE addition of
           exact inputs, so e_s = |fl32(s) - s| is known exactly (0 when
           the sum of the two bf16 values fits fp32, as in the constructed
           families).  Stored once: bf16 v |s| + (1 + v) e_s, fp32 e_s.
    mean : mean^ = p + fl(sum_i fl(s32_i - p)) / n with the pivot
           p = s32_0.  Each addend is off by u |s_i - p| + e_s_i + e_s_0,
           the sum of the k-deep tree by gamma_k sum |addend|, the
           division and the final add by u each (gamma_{k+2} in all on the
           addends, 2u on |mean|), and the e_s_i themselves by their mean.
    rstd : d_i = fl(s32_i - mean^) = (s_i - mean) - dm + h_i with
           |dm| <= E_mean and |h_i| <= e_s_i + u (|s_i - mean| + E_mean).
           sum_i (s_i - mean) dm = 0 exactly, so
             |mean d^2 - var| <= E_mean^2 + mean h^2 + 2 mean(|s - mean| h)
                                 + 2 E_mean mean h            =: dvar
           and the fp32 evaluation (square, k-deep sum, divide, + eps)
           adds gamma_{k+3} relative.  rsqrtf is within 1 ulp (HIP's
           documented accuracy), 2u relative.  With r the relative error
           of var + eps, rstd is off by rstd (r / (2 (1 - r)) + 2u).
    out  : (n_i - mean^) rstd^ gamma + beta, four fp32 operations, then one
           rounding (v for bf16, u for fp32).  n_i is s32_i in the fast
           kernel, the STORED s in the generic one (bf16 with a residual:
           another v |s|).
    """
    n = x.shape[1]
    path = ln_fwd_path(n, bf16)
    k = path["depth"]
    s, mean, rstd = ref["s"], ref["mean"], ref["rstd"]
    u, v = U_F32, V_BF16
    e_s = (f32_round(s) - s).abs()
    addend = (s - s[:, :1]).abs() + e_s + e_s[:, :1]
    e_mean = (gamma_k(k + 2) * addend.mean(dim=1) + e_s.mean(dim=1) +
              2 * u * mean.abs())
    dev = (s - mean[:, None]).abs()
    h = e_s + u * (dev + e_mean[:, None])
    dvar = (e_mean ** 2 + (h * h).mean(dim=1) + 2 * (dev * h).mean(dim=1) +
            2 * e_mean * h.mean(dim=1))
    r = dvar / (ref["var"] + eps) * (1 + gamma_k(k + 3)) + gamma_k(k + 3)
    rel_rstd = r / (2 * (1 - r)) + 2 * u
    e_rstd = rstd * rel_rstd
    if bf16:
        e_sum = v * s.abs() + (1 + v) * e_s
    else:
        e_sum = e_s
    e_n = e_s
    if not path["fast"] and bf16 and res is not None:
        e_n = e_sum          # the generic bf16 kernel normalizes the stored s
    xg = (ref["xhat"] * gamma).abs()
    fp = (gamma.abs() * rstd[:, None] * (e_mean[:, None] + e_n) * (1 + 4 * u)
          + xg * (rel_rstd[:, None] + 4 * u) + 2 * u * (xg + beta.abs()))
    w = v if bf16 else u
    e_out = w * ref["out"].abs() + (1 + w) * fp
    return dict(mean=e_mean, rstd=e_rstd, rel_rstd=rel_rstd, out=e_out,
                s=e_sum)


def ln_bwd_bounds(ref, dy, x, gamma, mean, rstd, dadd, bf16):
    """Per-element bounds of the backward kernels against ln_bwd_ref (same
    x, mean, rstd, all exact inputs).  k = depth of a row sum
    (ln_bwd_path), n = cols, R = rows.

    xhat^ = fl(fl(x - mean) rstd): 2u |xhat|.  dyg = dy gamma: u |dyg| (exact
    for bf16 inputs).  A^ = sum dyg: gamma_{k+1} sum |dyg|.  B^ = sum dyg
    xhat: gamma_{k+3} sum |dyg xhat|.
    t = A + xhat B: E_t = E_A + |xhat| E_B + 2u |xhat B| + 2u (|A| + |xhat B|)
    o = (dyg - t fl(1/n)) rstd: rstd (E_t / n + 4u (|dyg| + (|A| + |xhat
    B|) / n)) + u |o|; adding dadd: u |o + dadd|.  dx is o rounded once.
    dgamma / dbeta / colsum: every order of summing R addends in fp32 is
    within gamma_R sum |addend| of the exact sum (registers across a
    wave's rows, partial rows, atomics: R is the true addend count);
    the addends dy xhat^ carry 3u each, those of colsum E_o each."""
    n = x.shape[1]
    rows = x.shape[0]
    k = ln_bwd_path(n, bf16)["depth"]
    u, v = U_F32, V_BF16
    xhat, dyg, a, b = ref["xhat"], ref["dyg"], ref["a"], ref["b"]
    e_a = gamma_k(k + 1) * dyg.abs().sum(dim=1, keepdim=True)
    e_b = gamma_k(k + 3) * (dyg * xhat).abs().sum(dim=1, keepdim=True)
    xb = (xhat * b).abs()
    e_t = e_a + xhat.abs() * e_b + 2 * u * xb + 2 * u * (a.abs() + xb)
    e_o = (rstd[:, None] * (e_t / n + 4 * u * (dyg.abs() + (a.abs() + xb) / n))
           + u * ref["dx_ln"].abs())
    if dadd is not None:
        e_o = e_o + u * ref["dx"].abs()
    w = v if bf16 else u
    e_dx = w * ref["dx"].abs() + (1 + w) * e_o
    gr = gamma_k(rows)
    e_dgamma = (gr + 3 * u) * (dy * xhat).abs().sum(dim=0)
    e_dbeta = gr * dy.abs().sum(dim=0)
    e_colsum = gr * (ref["dx"].abs() + e_o).sum(dim=0) + e_o.sum(dim=0)
    return dict(dx=e_dx, dgamma=e_dgamma, dbeta=e_dbeta, colsum=e_colsum)


def colsum_bounds(dy, bf16):
    """gamma_R sum |addend| for the fp32 sum of R rows in any order (stripe
    partials, then the stripes), and the one rounding of a bf16 result"""
    e = gamma_k(dy.shape[0]) * dy.abs().sum(dim=0)
    if bf16:
        e = V_BF16 * dy.sum(dim=0).abs() + (1 + V_BF16) * e
    return e


# ---- emulation: the same arithmetic in fp32 with the kernels' roundings ------
def _rnd(t, bf16):
    t = t.to(torch.bfloat16) if bf16 else t
    return t.to(F64)


def ln_emulate(x, res, gamma, beta, bf16, eps=LN_EPS):
    """ln_ref with the forward kernels' roundings: every operation in fp32
    (torch's fp32 sums reassociate, as the kernels' trees do), the pivot
    shift, the variance from squared deviations, the stored s and out
    rounded once, the generic bf16 kernel normalizing the stored s."""
    n = x.shape[1]
    fast = ln_fwd_path(n, bf16)["fast"]
    f = torch.float32
    s32 = x.to(f) if res is None else x.to(f) + res.to(f)
    piv = s32[:, :1]
    mean = (piv + (s32 - piv).sum(dim=1, keepdim=True) / n)
    d = s32 - mean
    rstd = torch.rsqrt((d * d).sum(dim=1, keepdim=True) / n +
                       torch.tensor(eps, dtype=f))
    stored = _rnd(s32, bf16)
    nin = s32
    if not fast and res is not None:
        nin = stored.to(f)
    out = (nin - mean) * rstd * gamma.to(f) + beta.to(f)
    return dict(mean=mean.squeeze(1).to(F64), rstd=rstd.squeeze(1).to(F64),
                out=_rnd(out, bf16), s=stored)


def ln_bwd_emulate(dy, x, gamma, mean, rstd, dadd, bf16):
    f = torch.float32
    n = x.shape[1]
    dy32, g32 = dy.to(f), gamma.to(f)
    m32, r32 = mean.to(f)[:, None], rstd.to(f)[:, None]
    xhat = (x.to(f) - m32) * r32
    dyg = dy32 * g32
    a = dyg.sum(dim=1, keepdim=True)
    b = (dyg * xhat).sum(dim=1, keepdim=True)
    inv_n = torch.tensor(1.0, dtype=f) / n
    o = (dyg - (a + xhat * b) * inv_n) * r32
    if dadd is not None:
        o = o + dadd.to(f)
    return dict(dx=_rnd(o, bf16), dgamma=(dy32 * xhat).sum(dim=0).to(F64),
                dbeta=dy32.sum(dim=0).to(F64), colsum=o.sum(dim=0).to(F64))


def colsum_emulate(dy, bf16):
    return _rnd(dy.to(torch.float32).sum(dim=0), bf16)


# ---- bias + GeLU -------------------------------------------------------------
GELU_K0 = 0.7978845608028654      # sqrt(2 / pi)
GELU_K1 = 0.044715
GELU_D2_MAX = 0.8   # >= max |gelu''| = sqrt(2/pi) at z = 0 (asserted on the CPU)


def gelu_tanh(z):
    """tanh-GeLU, 0.5 z (1 + tanh a), written with 0.5 (1 + tanh a) =
    sigmoid(2a): the same function, and in fp64 it keeps its relative
    accuracy on the negative tail, where 1 + tanh a cancels to 0"""
    return z * torch.sigmoid(2 * GELU_K0 * (z + GELU_K1 * z ** 3))


def gelu_tanh_grad(z, cubic=True):
    s = torch.sigmoid(2 * GELU_K0 * (z + GELU_K1 * z ** 3))
    q = 1.0 + 3.0 * GELU_K1 * z * z if cubic else 1.0
    return s + z * s * (1.0 - s) * 2 * GELU_K0 * q


def bias_gelu_ref(x, bias, dy):
    """out = gelu_tanh(x + bias), dx = dy gelu_tanh'(x + bias), dbias =
    sum_rows dx, in fp64"""
    z = x + bias
    g = gelu_tanh_grad(z)
    dx = dy * g
    return dict(z=z, out=gelu_tanh(z), g=g, dx=dx, dbias=dx.sum(dim=0))


def bias_gelu_bwd_lean(cols, bf16):
    """the bf16 backward with 512-column wave segments (sigmoid form);
    every other backward uses the fp32 tanh form"""
    return bf16 and cols % 512 == 0


def gelu_sweep():
    """every bf16 value with 2^-6 <= |z| <= 12, 0 and +-40"""
    mant = 1.0 + torch.arange(128, dtype=F64) / 128
    vals = torch.cat([mant * 2.0 ** e for e in range(-6, 4)])
    vals = vals[vals <= 12.0]
    return torch.cat([-vals.flip(0), torch.zeros(1, dtype=F64), vals,
                      torch.tensor([-40.0, 40.0], dtype=F64)])


def bias_gelu_inputs(rows, cols, dy_name="coherent", seed=0):
    """x, bias, dy (bf16-representable fp64).  randn, except that the
    leading elements (at most half of them, spread evenly over the sweep
    when it does not fit) are x = bf16(z - bias) for the z of gelu_sweep(),
    with +-40 always present: x + bias lands within one bf16 step of x of
    every sweep point, over both saturated ends of the sigmoid and the
    derivative's minimum near -0.75."""
    gen = torch.Generator().manual_seed(seed + 17 * rows + 4099 * cols)
    x = bf16_round(torch.randn(rows, cols, generator=gen, dtype=F64))
    bias = bf16_round(torch.randn(cols, generator=gen, dtype=F64))
    sweep = gelu_sweep()
    m = max(2, min(sweep.numel(), rows * cols // 2))
    pick = torch.linspace(0, sweep.numel() - 3, m - 2).round().long()
    zs = torch.cat([sweep[pick], sweep[-2:]])
    flat = x.reshape(-1)
    flat[:m] = bf16_round(zs - bias.repeat(rows)[:m])
    dy = dy_family(dy_name, rows, cols, gen)
    return dict(x=x, bias=bias, dy=dy, nsweep=m)


def _gelu_sigmoid_terms(z):
    """the lean path's s = 1 / (1 + 2^w), w = z (c0 + c1 z^2): relative
    error of s.  w carries 6u (two rounded constants, four operations); 2^w
    turns an absolute dw into ln2 dw relative and v_exp_f32 adds 2u;
    1 + e inherits that scaled by e / (1 + e) = 1 - s, plus u; v_rcp_f32
    2u more.  A result under the fp32 normal range may flush: TINY_F32
    absolute."""
    u = U_F32
    w = 2 * GELU_K0 * math.log2(math.e) * (z + GELU_K1 * z ** 3).abs()
    s = torch.sigmoid(2 * GELU_K0 * (z + GELU_K1 * z ** 3))
    rel_s = (1 - s) * (math.log(2.0) * 6 * u * w + 2 * u) + 3 * u
    return s, rel_s


def _gelu_tanh_terms(z):
    """the fp32 path's t = 1 - 2 / (E + 1), E = __expf(2a), a = k0 (z + k1
    z^3): ABSOLUTE error of t.  2a carries 6u relative; __expf multiplies
    by log2(e) and takes exp2 (2u more on the argument, 4u on the result):
    rel_E = 8u |2a| + 4u.  D = E + 1: E rel_E + u D.  Q = 2 / D, division
    within 3u: Q (E rel_E / D + 4u) with E / D = 1 - Q / 2.  t = 1 - Q:
    that plus u |t|.  Q is near 2 on the negative side: there t is -1 +
    O(E) computed with an absolute error of about 8u = 2^-21, which the
    outputs see as |z| 2^-22-scale absolute terms."""
    u = U_F32
    a2 = 2 * GELU_K0 * (z + GELU_K1 * z ** 3)
    t = torch.tanh(a2 / 2)
    q = 1 - t                       # Q = 2 / (E + 1) = 1 - t
    rel_e = 8 * u * a2.abs() + 4 * u
    e_t = q * ((1 - q / 2) * rel_e + 4 * u) + u * t.abs()
    return t, e_t


def bias_gelu_bounds(ref, x, bias, dy, bf16):
    """Per-element bounds against bias_gelu_ref.  z^ = fl(x + bias): u |z|,
    which moves gelu by u |z gelu'| and gelu' by u |z| GELU_D2_MAX.

    bf16 forward, out = z s:  |out| (rel_s + 2u) + u |z gelu'| + |z| TINY,
      then one bf16 rounding.
    bf16 backward with 512-column segments, g = s + z s (1 - s) q,
      q = d0 + d1 z^2 (3u):  1 - s is off by s rel_s + u (1 - s), so
      E_g = s rel_s + |z s q| (s rel_s + u (1 - s)) + |P| (rel_s + 6u)
            + u |g| + u |z| GELU_D2_MAX,  P = z s (1 - s) q.
    fp32 form (fp32 tensors, and the bf16 backward at other widths):
      out = 0.5 z (1 + t):  0.5 |z| (E_t + u (1 + t)) + 2u |out| + u |z gelu'|
      1 - t^2: 2 |t| E_t + 2u;  dt = (1 - t^2) k0 (1 + 3 k1 z^2):
      k0 (1 + 3 k1 z^2) (2 |t| E_t + 2u) + 5u |dt|
      E_g = 0.5 (E_t + u (1 + t)) + 0.5 |z| E_dt + 3u (0.5 (1 + t)
            + 0.5 |z dt|) + u |z| GELU_D2_MAX.
    dx = dy g rounded once; dbias = sum over R rows of the unrounded dy g:
    gamma_R sum |dy g| + sum |dy| E_g (+ the u per product).
    """
    u, v = U_F32, V_BF16
    z, g = ref["z"], ref["g"]
    rows, cols = x.shape
    zd1 = u * (z * g).abs()
    zd2 = u * z.abs() * GELU_D2_MAX
    s, rel_s = _gelu_sigmoid_terms(z)
    t, e_t = _gelu_tanh_terms(z)
    if bf16:
        fp = ref["out"].abs() * (rel_s + 2 * u) + zd1 + z.abs() * TINY_F32
        e_out = v * ref["out"].abs() + (1 + v) * fp
    else:
        e_out = (0.5 * z.abs() * (e_t + u * (1 + t)) +
                 3 * u * ref["out"].abs() + zd1)
    if bias_gelu_bwd_lean(cols, bf16):
        q = 2 * GELU_K0 * (1 + 3 * GELU_K1 * z * z)
        p = z * s * (1 - s) * q
        e_g = (s * rel_s + (z * s * q).abs() * (s * rel_s + u * (1 - s)) +
               p.abs() * (rel_s + 6 * u) + u * g.abs() + zd2 + TINY_F32)
    else:
        kq = GELU_K0 * (1 + 3 * GELU_K1 * z * z)
        dt = (1 - t * t) * kq
        e_dt = kq * (2 * t.abs() * e_t + 2 * u) + 5 * u * dt.abs()
        e_g = (0.5 * (e_t + u * (1 + t)) + 0.5 * z.abs() * e_dt +
               3 * u * (0.5 * (1 + t) + 0.5 * (z * dt).abs()) + zd2)
    e_prod = dy.abs() * e_g + u * ref["dx"].abs()
    w = v if bf16 else u
    e_dx = w * ref["dx"].abs() + (1 + w) * e_prod
    e_dbias = (gamma_k(rows) * (ref["dx"].abs() + e_prod).sum(dim=0) +
               e_prod.sum(dim=0))
    return dict(out=e_out, dx=e_dx, dbias=e_dbias)


def bias_gelu_emulate(x, bias, dy, bf16):
    """bias_gelu_ref in fp32 with the kernels' formulas and roundings"""
    f = torch.float32
    cols = x.shape[1]
    z = x.to(f) + bias.to(f)
    dy32 = dy.to(f)
    k0, k1 = GELU_K0, GELU_K1
    log2e = 1.4426950408889634

    def sig(z):
        c0 = torch.tensor(-2.0 * k0 * log2e, dtype=f)
        c1 = torch.tensor(-2.0 * k0 * log2e * k1, dtype=f)
        return 1.0 / (1.0 + torch.exp2(z * (c0 + c1 * z * z)))

    def tanh_fast(a):
        return 1.0 - 2.0 / (torch.exp(2.0 * a) + 1.0)

    def arg(z):
        return torch.tensor(k0, dtype=f) * (z + torch.tensor(k1, dtype=f)
                                            * z * z * z)

    if bf16:
        out = z * sig(z)
    else:
        out = 0.5 * z * (1.0 + tanh_fast(arg(z)))
    if bias_gelu_bwd_lean(cols, bf16):
        s = sig(z)
        d0 = torch.tensor(2.0 * k0, dtype=f)
        d1 = torch.tensor(6.0 * k0 * k1, dtype=f)
        g = s + z * s * (1.0 - s) * (d0 + d1 * z * z)
    else:
        t = tanh_fast(arg(z))
        dt = (1.0 - t * t) * torch.tensor(k0, dtype=f) * (
            1.0 + 3.0 * torch.tensor(k1, dtype=f) * z * z)
        g = 0.5 * (1.0 + t) + 0.5 * z * dt
    dx = dy32 * g
    return dict(out=_rnd(out, bf16), dx=_rnd(dx, bf16),
                dbias=dx.sum(dim=0).to(F64))


# ---- the GPU matrix (test_layer_norm_fp64_gpu.py, test_bias_gelu_fp64_gpu.py;
# test_kernel_refs_cpu.py proves the bounds on the same cases) ---------------
LN_FAST_COLS = (8, 64, 504, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056,
                3000, 4096)
LN_GENERIC_COLS = (4104, 8192)
LN_F32_COLS = (1000, 1024)
LN_ROWS = (1, 3, 37)
LN_GRID_CASES = ((64, 4099), (512, 8191), (1600, 8191))    # (cols, rows)
LN_FLAGS = ((False, False), (True, False), (False, True), (True, True))
LN_FACTOR_BF16 = dict(out=2.0, s=2.0, dx=2.0, mean=1.0, rstd=1.0,
                      dgamma=1.0, dbeta=1.0, colsum=1.0)
LN_FACTOR_F32 = dict(LN_FACTOR_BF16, out=1.0, s=1.0, dx=1.0)


def ln_cases():
    """(cols, rows, bf16) of the GPU matrix"""
    cases = [(c, r, True) for c in LN_FAST_COLS + LN_GENERIC_COLS
             for r in LN_ROWS]
    cases += [(c, r, False) for c in LN_F32_COLS for r in LN_ROWS]
    cases += [(c, r, True) for c, r in LN_GRID_CASES]
    return cases


def ln_rots(rows):
    """row-kind rotations one shape runs: every kind is met at every
    shape (13 launches of one row, 5 of three, one of 37 or more)"""
    nk = len(LN_KINDS)
    return tuple(range(0, nk, rows)) if rows < nk else (0,)


def ln_dy_names(rows, rot):
    """both dy families on the small shapes; the grid-stride shapes keep
    their fp64 reference to one"""
    if rows > 1000:
        return ("cancel",) if rows % 2 else ("coherent",)
    return LN_DY_FAMILIES if rot == 0 else (LN_DY_FAMILIES[(rot // 3) % 2],)


GELU_BF16_COLS = (8, 24, 512, 520, 1024, 1536, 4096)
GELU_ROWS = (1, 3, 37, 1025)
GELU_F32_SHAPES = ((37, 24), (256, 512), (1025, 1000))
GELU_FACTOR_BF16 = dict(out=2.0, dx=2.0, dbias=1.0)
GELU_FACTOR_F32 = dict(out=1.0, dx=1.0, dbias=1.0)


def gelu_cases():
    """(rows, cols, bf16)"""
    return ([(r, c, True) for c in GELU_BF16_COLS for r in GELU_ROWS] +
            [(r, c, False) for r, c in GELU_F32_SHAPES])


COLSUM_COLS = (8, 1024, 3072)
COLSUM_ROWS = (1, 5, 4099)


def guarded_rows(rows, cols, dtype, device):
    """[rows, cols] output behind two guard rows on either side"""
    return GuardedBuffer((rows, cols), (cols, 1), 0, dtype, device,
                         2 * cols + 16)


def ln_check_case(cols, rows, bf16, fwd_fn, bwd_fn, factor):
    """Run one (cols, rows, dtype) case of the LayerNorm matrix through
    ``fwd_fn(inp, with_res) -> dict(mean, rstd, out[, s])`` and
    ``bwd_fn(inp, x_used, mean, rstd, dadd, want_colsum) -> dict(dx,
    dgamma, dbeta[, colsum])`` (fp64 results) and compare with the
    references: forward with and without a residual, every rotation of the
    row kinds, then the backward at the forward's own s / mean / rstd for
    the dy families and the (dadd, colsum) combinations the shape has.
    Returns (worst, bad): worst[output][family] = largest err / E (the
    forward per row family, the backward per dy family), bad = the text
    of every result over factor[output] x E."""
    worst, bad = {}, []

    def note(name, family, r, label):
        slot = worst.setdefault(name, {})
        slot[family] = max(slot.get(family, 0.0), r)
        if not r <= factor[name]:
            bad.append("{} {} {}: err/E {:.3g} > {}".format(
                label, name, family, r, factor[name]))

    fams = [LN_KINDS[k][1] for k in range(len(LN_KINDS))]
    fast_bwd = ln_bwd_path(cols, bf16)["fast"]
    for rot in ln_rots(rows):
        for with_res in (False, True):
            inp = ln_inputs(rows, cols, with_res, rot=rot)
            label = "res%d rot%d" % (with_res, rot)
            ref = ln_ref(inp["x"], inp["res"], inp["gamma"], inp["beta"])
            e = ln_fwd_bounds(ref, inp["x"], inp["res"], inp["gamma"],
                              inp["beta"], bf16)
            assert float((e["rel_rstd"]).max()) <= LN_RSTD_REL_MAX
            got = fwd_fn(inp, with_res)
            names = ("mean", "rstd", "out") + (("s",) if with_res else ())
            for k in sorted(set(inp["kinds"].tolist())):
                sel = inp["kinds"] == k
                for name in names:
                    note(name, fams[k], ratio_of(
                        got[name][sel], ref[name][sel], e[name][sel]), label)
            finite = all(bool(torch.isfinite(got[n]).all()) for n in names)
            if not finite:
                bad.append(label + " forward not finite")
                continue    # nothing to hand to the backward
            x_used = got["s"] if with_res else inp["x"]
            for dy_name in ln_dy_names(rows, rot):
                gen = torch.Generator().manual_seed(rot + 5 * cols + rows)
                dy = dy_family(dy_name, rows, cols, gen)
                bref = {}
                for use_dadd, use_cs in (LN_FLAGS if fast_bwd else
                                         LN_FLAGS[:1]):
                    dadd = inp["dadd"] if use_dadd else None
                    if use_dadd not in bref:
                        r = ln_bwd_ref(dy, x_used, inp["gamma"], got["mean"],
                                       got["rstd"], dadd)
                        bref[use_dadd] = (r, ln_bwd_bounds(
                            r, dy, x_used, inp["gamma"], got["mean"],
                            got["rstd"], dadd, bf16))
                    r, eb = bref[use_dadd]
                    res = bwd_fn(dict(inp, dy=dy), x_used, got["mean"],
                                 got["rstd"], dadd, use_cs)
                    lab = "%s %s dadd%d cs%d" % (label, dy_name, use_dadd,
                                                 use_cs)
                    for name in ("dx", "dgamma", "dbeta") + (
                            ("colsum",) if use_cs else ()):
                        note(name, dy_name, ratio_of(res[name], r[name],
                                                     eb[name]), lab)
    return worst, bad


def gelu_check_case(rows, cols, bf16, fn, factor):
    """one (rows, cols, dtype) case of the bias-GeLU matrix through
    ``fn(inp) -> dict(out, dx, dbias)``, for both dy families"""
    worst, bad = {}, []
    for dy_name in LN_DY_FAMILIES:
        inp = bias_gelu_inputs(rows, cols, dy_name)
        ref = bias_gelu_ref(inp["x"], inp["bias"], inp["dy"])
        e = bias_gelu_bounds(ref, inp["x"], inp["bias"], inp["dy"], bf16)
        got = fn(inp)
        for name in ("out", "dx", "dbias"):
            r = ratio_of(got[name], ref[name], e[name])
            slot = worst.setdefault(name, {})
            slot[dy_name] = max(slot.get(dy_name, 0.0), r)
            if not r <= factor[name]:
                bad.append("{} {}: err/E {:.3g} > {}".format(
                    dy_name, name, r, factor[name]))
    return worst, bad


def format_worst(worst):
    return " ".join("{}[{}]".format(name, ",".join(
        "{}={:.3f}".format(f, r) for f, r in sorted(fams.items())))
        for name, fams in worst.items())
