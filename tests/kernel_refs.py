"""Plain fp64 references and deterministic input builders for the HIP
kernel tests (LAMB phases, sharded cross-entropy, MoE dispatch/combine,
flash attention with its derived per-element rounding bounds).

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
