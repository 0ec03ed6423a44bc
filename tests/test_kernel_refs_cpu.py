"""The fp64 references and input builders of kernel_refs.py, validated
without a GPU: each reference against an independent torch formulation,
and each builder against the properties the GPU tests rely on."""

import pytest
import torch

from tests import kernel_refs as kr

F64 = torch.float64


# ---- LAMB -----------------------------------------------------------------
def _cpu_lamb_group(dtype=torch.float32):
    from easyparallellibrary_amd.parallel.dp import FlatParamGroup
    from easyparallellibrary_amd.runtime.optim import FusedLAMB
    params = kr.lamb_params(dtype=dtype)
    g = FlatParamGroup(params, torch.device("cpu"))
    return g, FusedLAMB


@pytest.mark.parametrize("wd", [0.01, 0.0])
@pytest.mark.parametrize("grad_scale", [1.0, 1024.0])
def test_lamb_ref_matches_step_torch(wd, grad_scale):
    g, FusedLAMB = _cpu_lamb_group()
    opt = FusedLAMB([g], lr=1e-2, weight_decay=wd)
    ext = kr.lamb_extents(g)
    mag = kr.lamb_elem_magnitude(g)
    kr.lamb_fill(g, seed=10, scale_weights=True, grad_mul=0.0)
    master = g.master_arena.to(F64).clone()
    m = torch.zeros_like(master)
    v = torch.zeros_like(master)
    for step in (1, 2, 3):
        kr.lamb_fill(g, seed=10 + step, grad_mul=grad_scale,
                     zero_grad_chunk=1 if step == 1 else None)
        r = kr.lamb_ref(master, g.grad_arena.to(F64), m, v, ext, opt.lr,
                        opt.beta1, opt.beta2, opt.eps, wd, step,
                        1.0 / grad_scale)
        opt.step(grad_scale=grad_scale)
        # the zero parameter has ||w|| = 0 at step 1; at wd = 0 the
        # zero-gradient parameter has ||u|| = 0: both take ratio 1
        if step == 1:
            zc = [c for c, (o, n) in enumerate(ext)
                  if not master[o:o + n].any()]
            assert len(zc) == 1 and r["wsq"][zc[0]] == 0
            assert r["ratio"][zc[0]] == 1.0
            if wd == 0.0:
                assert r["usq"][1] == 0 and r["ratio"][1] == 1.0
                assert torch.equal(r["master"][ext[1][0]:sum(ext[1])],
                                   master[ext[1][0]:sum(ext[1])])
        tol = 1e-6 * mag + 1e-5 * r["master"].abs()
        assert ((g.master_arena.to(F64) - r["master"]).abs() <= tol).all()
        assert ((g.state["exp_avg"].to(F64) - r["m"]).abs()
                <= 1e-6 * mag + 1e-5 * r["m"].abs()).all()
        assert ((g.state["exp_avg_sq"].to(F64) - r["v"]).abs()
                <= 1e-6 * mag + 1e-5 * r["v"]).all()
        master, m, v = r["master"], r["m"], r["v"]


def test_lamb_ref_known_values():
    """One element, hand-computed: step 1 gives mhat = g, vhat = g^2."""
    master = torch.tensor([2.0, -1.0], dtype=F64)
    grad = torch.tensor([3.0, 0.5], dtype=F64) * 8
    z = torch.zeros(2, dtype=F64)
    r = kr.lamb_ref(master, grad, z, z, [(0, 1), (1, 1)], 0.1, 0.9, 0.999,
                    0.0, 0.5, 1, 1 / 8)
    u = torch.tensor([1.0 + 0.5 * 2.0, 1.0 - 0.5], dtype=F64)
    assert torch.allclose(r["update"], u, rtol=1e-12)
    assert torch.allclose(r["ratio"], torch.tensor([1.0, 2.0], dtype=F64),
                          rtol=1e-12)
    assert torch.allclose(r["master"], master - 0.1 * r["ratio"] * u,
                          rtol=1e-12)


def test_lamb_chunk_map_covers_padding():
    """chunk_of is read for padding elements as well and indexes the norm
    buffers: no entry may be left unset."""
    g, FusedLAMB = _cpu_lamb_group(torch.bfloat16)
    FusedLAMB([g])
    kr.check_chunk_map(g)
    # the arena the GPU tests use: padded extents, 128-aligned
    assert [e for _, e in kr.lamb_padded_extents(g)] == \
        [4096, 384, 128, 2176, 256, 128]
    assert g.master_arena is not g.param_arena


# ---- cross-entropy --------------------------------------------------------
CE_CASES = [(5, [8]), (5, [7]), (37, [2048, 2056, 1001]), (1, [264, 264]),
            (4097, [264, 256])]


@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_ce_ref_matches_torch(ignore_index):
    logits, targets, dloss, _ = kr.ce_case(37, [40, 48, 9], F64,
                                           ignore_index)
    loss, dlogits = kr.ce_ref(logits, targets, ignore_index, dloss, 0.5)
    lr = logits.clone().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(
        lr, targets, ignore_index=ignore_index, reduction="none")
    want.backward(dloss.to(F64) * 0.5)
    assert torch.allclose(loss, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dlogits, lr.grad, rtol=1e-12, atol=1e-14)
    ign = targets == ignore_index
    assert ign.any() and (loss[ign] == 0).all()
    assert (dlogits[ign] == 0).all()


def test_ce_shard_stats_merge_to_full_loss():
    widths = [40, 48, 9]
    logits, targets, _, _ = kr.ce_case(37, widths, F64)
    loss, _ = kr.ce_ref(logits, targets, -100)
    stats, b = [], 0
    for w in widths:
        stats.append(kr.ce_shard_stats_ref(logits[:, b:b + w], targets, b,
                                           -100))
        b += w
    gmax = torch.stack([s[0] for s in stats]).max(dim=0).values
    gsum = sum(s[1] * torch.exp(s[0] - gmax) for s in stats)
    tl = sum(s[2] for s in stats)
    merged = torch.where(targets != -100, gsum.log() + gmax - tl,
                         torch.zeros_like(gmax))
    assert torch.allclose(merged, loss, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("rows,widths", CE_CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ce_case_properties(rows, widths, dtype):
    ignore_index = 0 if rows == 37 else -100
    logits, targets, dloss, special = kr.ce_case(rows, widths, dtype,
                                                 ignore_index)
    vocab = sum(widths)
    assert logits.shape == (rows, vocab) and logits.dtype == dtype
    live = targets != ignore_index
    assert int(targets[live].min()) >= 0 and int(targets[live].max()) < vocab
    assert (targets[6::7] == ignore_index).all()
    req = kr.ce_required_targets(widths)
    n_live = sum(1 for r in range(rows) if r % 7 != 6)
    for t in req[:n_live]:
        assert (targets == t).any(), t
    if rows >= 7:
        # both sides of every shard edge, the last column, class 0
        assert len(req) == 2 * len(widths) and len(req) <= n_live
    lf = logits.to(F64)
    plain = torch.ones(rows, dtype=torch.bool)
    for r in special.values():
        plain[r] = False
    assert lf[plain].abs().max() <= 8
    if "hot" in special:
        assert lf[special["hot"]].min() >= 96
    if "equal" in special:
        assert (lf[special["equal"]] == lf[special["equal"]][0]).all()
    for name, gap in (("gap60", 60), ("gap120", 120)):
        if name in special:
            r = special[name]
            others = lf[r, widths[0]:].max()
            # bf16 rounds the peak by up to 2**-8 relative
            assert lf[r, kr.CE_PEAK_COL] - others >= gap - 0.5
            assert targets[r] != kr.CE_PEAK_COL
    if len(widths) > 1 and rows > kr.CE_GAP120:
        assert set(special) == {"hot", "gap60", "equal", "gap120"}
        # the far shards' rescaled sum is 0 in fp32 for the wide gap
        assert torch.exp(torch.tensor(-119.5, dtype=torch.float32)) \
            * vocab == 0
    assert dloss.dtype == torch.float32
    assert dloss.unique().numel() > rows // 2      # non-uniform


# ---- MoE ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kr.MOE_PATTERNS))
def test_moe_pattern_properties(name):
    pattern, k, cap = kr.MOE_PATTERNS[name]
    fe, pos, ft, inv, fw = kr.moe_assignment(96, k, 4, cap, pattern)
    kr.moe_check_claims(name, fe, pos, ft, inv, k, 4, cap, 96)
    assert fw.dtype == torch.float32 and fw.unique().numel() == fw.numel()
    assert fw.min() > 0.1 and fw.max() < 0.9


@pytest.mark.parametrize("pattern,k,cap", [("uneven1", 1, 20000),
                                           ("skew", 2, 40000)])
def test_moe_grid_stride_lists(pattern, k, cap):
    n = 70000
    fe, pos, ft, inv, fw = kr.moe_assignment(n, k, 4, cap, pattern)
    kr.moe_check_lists(fe, pos, ft, inv, k, 4, n)
    props = kr.moe_properties(fe, pos, ft, k, 4, cap, n)
    assert n > 65536 and props["dropped"] > 0
    assert fw.unique().numel() > n // 2   # fp32 spacing merges a few


@pytest.mark.parametrize("top_k,cf", [(2, 1.25), (2, 0.5), (1, 0.25)])
def test_moe_refs_match_module_torch_path(top_k, cf):
    """dispatch ref -> expert FFN -> combine ref equals ExpertParallelMLP's
    torch index path (what EPL_MOE_NATIVE_DISPATCH=0 computes), fp64."""
    import easyparallellibrary_amd as epl
    from easyparallellibrary_amd.ops.moe import ExpertParallelMLP
    epl.init()
    torch.manual_seed(0)
    hidden, ffn, E, n = 16, 24, 4, 40
    mod = ExpertParallelMLP(hidden, ffn, E, top_k=top_k,
                            capacity_factor=cf).double()
    x = torch.randn(n, hidden, dtype=F64)
    with torch.no_grad():
        want = mod(x)
        probs = mod.gate(x).float().softmax(dim=-1)
        topv, topi = probs.topk(top_k, dim=-1)
        topv = topv / topv.sum(dim=-1, keepdim=True)
        cap = max(1, int(cf * n * top_k / E))
        fe, pos, ft, inv, order = kr.moe_assignment_from_topi(topi, E)
        kr.moe_check_lists(fe, pos, ft, inv, top_k, E, n)
        fw = topv.reshape(-1)[order]
        if cf < 1:
            assert (pos >= cap).any()
        disp, written = kr.moe_dispatch_fwd_ref(x, fe, pos, ft, E, cap)
        assert (disp[~written] == 0).all()
        h = torch.stack([
            torch.nn.functional.gelu(disp[e] @ mod.w1[e]) @ mod.w2[e]
            for e in range(E)])
        out, _ = kr.moe_combine_fwd_ref(h, fw, fe, pos, ft, n, cap)
    assert torch.allclose(out, want, rtol=1e-10, atol=1e-12)


def test_moe_backward_refs_are_the_adjoints():
    """<dispatch(x), g> = <x, dispatch_bwd(g)>, and combine_bwd is the
    gradient of <combine(h, fw), dout> by autograd."""
    n, k, E, cap, hidden = 96, 2, 4, 10, 8
    fe, pos, ft, inv, fw = kr.moe_assignment(n, k, E, cap, "skew")
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(n, hidden, generator=gen, dtype=F64)
    g = torch.randn(E, cap, hidden, generator=gen, dtype=F64)
    disp, _ = kr.moe_dispatch_fwd_ref(x, fe, pos, ft, E, cap)
    dx = kr.moe_dispatch_bwd_ref(g, fe, pos, ft, n, cap)
    assert torch.allclose((disp * g).sum(), (x * dx).sum(), rtol=1e-12)

    h = torch.randn(E, cap, hidden, generator=gen,
                    dtype=F64).requires_grad_(True)
    fwd = fw.to(F64).requires_grad_(True)
    dout = torch.randn(n, hidden, generator=gen, dtype=F64)
    keep = pos < cap
    out = torch.zeros(n, hidden, dtype=F64).index_add(
        0, ft[keep], h[fe[keep], pos[keep]] * fwd[keep][:, None])
    ref_out, _ = kr.moe_combine_fwd_ref(h.detach(), fw, fe, pos, ft, n, cap)
    assert torch.allclose(out.detach(), ref_out, rtol=1e-12)
    out.backward(dout)
    dh, dfw, _ = kr.moe_combine_bwd_ref(dout, h.detach(), fw, fe, pos, ft,
                                        E, cap)
    assert torch.allclose(dh, h.grad, rtol=1e-12, atol=1e-14)
    assert torch.allclose(dfw, fwd.grad, rtol=1e-12, atol=1e-14)
    assert (dfw[~keep] == 0).all()


# ---- flash attention ---------------------------------------------------------
def _cpu_keep(seq, thresh, seed=0):
    """Bernoulli keep bits at the kernel's rate 1 - thresh/256"""
    if not thresh:
        return None
    gen = torch.Generator().manual_seed(900 + seed + seq + thresh)
    u = torch.rand(kr.ATTN_B, kr.ATTN_H, seq, seq, generator=gen, dtype=F64)
    return (u >= thresh / 256.0).to(F64)


def _attn_case(family, seq, d, causal, thresh=0, with_dlse=False):
    q, k, v, dout = kr.attn_inputs(family, seq, d, causal)
    keep = _cpu_keep(seq, thresh)
    dlse = kr.attn_dlse(seq) if with_dlse else None
    return q, k, v, dout, d ** -0.5, keep, kr.attn_inv_keep(thresh), dlse


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("family", kr.ATTN_FAMILIES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("thresh,with_dlse", [(0, False), (128, True)])
def test_attn_ref_matches_autograd(family, causal, thresh, with_dlse):
    for seq, d in ((1, 64), (33, 128), (72, 64), (129, 64)):
        q, k, v, dout, scale, keep, inv_keep, dlse = _attn_case(
            family, seq, d, causal, thresh, with_dlse)
        ref = kr.attn_ref(q, k, v, dout, causal, scale, keep, inv_keep,
                          dlse)
        qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
        s = torch.matmul(qa, ka.transpose(-1, -2)) * scale
        if causal:
            s = s.masked_fill(torch.triu(torch.ones(
                seq, seq, dtype=torch.bool), 1), float("-inf"))
        p = torch.softmax(s, dim=-1)
        if keep is not None:
            p = p * keep * inv_keep
        out = torch.matmul(p, va)
        lse = torch.logsumexp(s, dim=-1)
        dl = dlse if dlse is not None else torch.zeros_like(lse)
        gq, gk, gv = torch.autograd.grad([out, lse], [qa, ka, va],
                                         [dout, dl])
        for name, want in (("out", out.detach()), ("lse", lse.detach()),
                           ("dq", gq), ("dk", gk), ("dv", gv)):
            assert _rel(ref[name], want) < 1e-12, (name, seq, d)
        if keep is None:
            sdpa = torch.nn.functional.scaled_dot_product_attention(
                q, k, v, is_causal=causal, scale=scale)
            assert _rel(ref["out"], sdpa) < 1e-12, (seq, d)


def test_attn_input_families_have_their_properties():
    for d in kr.ATTN_DIMS:
        for seq in (72, 200, 257):
            for causal in (False, True):
                scale = d ** -0.5
                for family in kr.ATTN_FAMILIES:
                    ts = kr.attn_inputs(family, seq, d, causal)
                    for t in ts:     # exactly representable in bf16
                        assert t.shape == (kr.ATTN_B, kr.ATTN_H, seq, d)
                        assert torch.equal(kr.bf16_round(t), t)
                    again = kr.attn_inputs(family, seq, d, causal)
                    assert all(torch.equal(a, b) for a, b in zip(ts, again))
                q, k, v, dout = kr.attn_inputs("peaked", seq, d, causal)
                ref = kr.attn_ref(q, k, v, dout, causal, scale)
                assert 30 < float(ref["s"].abs().max()) < 60
                pairs = kr.attn_peak_pairs(seq, causal)
                keys = {key for _, key in pairs}
                assert keys >= {0, 31, 32, 63, 64, seq - 1}
                assert (127 in keys and 128 in keys) or seq <= 128
                if causal:
                    assert any(r == key for r, key in pairs)
                    assert any(r == key + 1 for r, key in pairs)
                for row, key in pairs:
                    assert not causal or key <= row
                    assert float(ref["P"][:, :, row, key].min()) > 0.9
                q, k, v, dout = kr.attn_inputs("shifted", seq, d, causal)
                s = kr.attn_ref(q, k, v, dout, False, scale)["s"]
                mean = s.mean(dim=-1)
                assert float(mean.max()) > 50 and float(mean.min()) < -50
                assert float(mean.abs().min()) > 40
                assert float(s.std(dim=-1).max()) < 6


def _emulation_ratios(case):
    q, k, v, dout, scale, keep, inv_keep, dlse = case[:8]
    causal = case[8]
    ref = kr.attn_ref(q, k, v, dout, causal, scale, keep, inv_keep, dlse)
    bounds = kr.attn_bounds(ref, q, k, v, dout, scale)
    emu = kr.attn_emulate(q, k, v, dout, causal, scale, keep, inv_keep, dlse)
    ratios = {}
    for name in kr.ATTN_OUTPUTS:
        want, bound = ref[name], bounds[name]
        if name == "delta":
            want, bound = kr.attn_delta_ref(dout, emu["delta_from"], dlse)
        ratios[name] = kr.attn_ratio((emu[name] - want).abs(), bound)
    return ratios


def _assert_emulation_inside(label, case, worst):
    for name, r in _emulation_ratios(case).items():
        worst[name] = max(worst.get(name, 0.0), r)
        assert r <= 1.0, (label, name, r)


@pytest.mark.parametrize("family", kr.ATTN_FAMILIES)
@pytest.mark.parametrize("d", kr.ATTN_DIMS)
@pytest.mark.parametrize("causal", [False, True])
def test_attn_emulation_inside_bounds_main(family, d, causal):
    worst = {}
    for seq in kr.ATTN_SEQS:
        _assert_emulation_inside(
            (seq,), _attn_case(family, seq, d, causal) + (causal,), worst)
    print(family, d, causal, worst)


@pytest.mark.parametrize("thresh", sorted(kr.ATTN_DROP_FAMILY))
@pytest.mark.parametrize("d", kr.ATTN_DIMS)
@pytest.mark.parametrize("causal", [False, True])
def test_attn_emulation_inside_bounds_dropout(thresh, d, causal):
    worst = {}
    # threshold 128 also runs on randn (the garbage-bit test)
    families = kr.ATTN_FAMILIES if thresh == 128 else (
        kr.ATTN_DROP_FAMILY[thresh],)
    for seq in kr.ATTN_DROP_SEQS:
        for family in families:
            _assert_emulation_inside(
                (seq, family), _attn_case(family, seq, d, causal, thresh) +
                (causal,), worst)
    print(thresh, d, causal, worst)


@pytest.mark.parametrize("d", kr.ATTN_DIMS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("thresh", [0, 128])
def test_attn_emulation_inside_bounds_dlse(d, causal, thresh):
    worst = {}
    for seq in kr.ATTN_DLSE_SEQS:
        for family in kr.ATTN_FAMILIES:
            _assert_emulation_inside(
                (seq, family), _attn_case(family, seq, d, causal, thresh,
                                          True) + (causal,), worst)
    print(d, causal, thresh, worst)


def test_attn_emulation_inside_bounds_env_cases():
    worst = {}
    for d, seq, causal, thresh, family in kr.attn_env_cases(0):
        _assert_emulation_inside(
            (d, seq, causal, thresh, family),
            _attn_case(family, seq, d, causal, thresh) + (causal,), worst)
    print(worst)


ATTN_MUTATIONS = (
    "causal_ge", "last_key_dropped", "padding_key_counted",
    "v_rows_exchanged", "bh_transposed", "keep_from_neighbour_key",
    "dp_without_inv_keep", "dropout_in_normaliser", "dlse_dropped",
    "dlse_negated", "lse_without_last_tile")


def _attn_mutants(q, k, v, dout, causal, scale, keep, inv_keep, dlse, ref):
    """wrong kernels, as outputs of a mutated reference: name -> outputs"""
    b, h, seq, _ = q.shape
    kt = lambda t: t.transpose(-1, -2)
    m = {}
    if causal:
        # masks kv >= q instead of kv > q; row 0 keeps its only key
        valid = torch.tril(torch.ones(seq, seq, dtype=torch.bool), -1)
        valid[0, 0] = True
        m["causal_ge"] = kr.attn_ref(q, k, v, dout, causal, scale, keep,
                                     inv_keep, dlse, valid=valid)
    valid = ref["valid"].clone()
    valid[:, seq - 1] = False
    m["last_key_dropped"] = kr.attn_ref(q, k, v, dout, causal, scale, keep,
                                        inv_keep, dlse, valid=valid)
    if not causal:
        ext = lambda t, dim: torch.cat(
            [t, t.narrow(dim, t.shape[dim] - 1, 1)], dim)
        r = kr.attn_ref(q, ext(k, 2), ext(v, 2), dout, False, scale,
                        None if keep is None else ext(keep, 3), inv_keep,
                        dlse)
        m["padding_key_counted"] = dict(
            r, dk=r["dk"][:, :, :seq], dv=r["dv"][:, :, :seq])
    j = seq // 2
    v2 = v.clone()
    v2[:, :, [j, j + 1]] = v[:, :, [j + 1, j]]
    m["v_rows_exchanged"] = kr.attn_ref(q, k, v2, dout, causal, scale, keep,
                                        inv_keep, dlse)
    idx = [(bh % b) * h + bh // b for bh in range(b * h)]
    fl = lambda t: t.reshape(b * h, seq, -1)[idx].reshape(t.shape)
    m["bh_transposed"] = kr.attn_ref(fl(q), fl(k), fl(v), fl(dout), causal,
                                     scale, keep, inv_keep, dlse)
    if keep is not None:
        m["keep_from_neighbour_key"] = kr.attn_ref(
            q, k, v, dout, causal, scale, torch.roll(keep, 1, -1), inv_keep,
            dlse)
        dp = torch.matmul(dout, kt(v)) * keep
        ds = ref["P"] * (dp - ref["delta"].unsqueeze(-1)) * scale
        m["dp_without_inv_keep"] = dict(dq=torch.matmul(ds, k),
                                        dk=torch.matmul(kt(ds), q))
        e = ref["P"] * keep
        m["dropout_in_normaliser"] = dict(out=torch.matmul(
            e / e.sum(dim=-1, keepdim=True).clamp_min(1e-300), v))
    if dlse is not None:
        m["dlse_dropped"] = kr.attn_ref(q, k, v, dout, causal, scale, keep,
                                        inv_keep, None)
        m["dlse_negated"] = kr.attn_ref(q, k, v, dout, causal, scale, keep,
                                        inv_keep, -dlse)
    if seq > 64:
        valid = ref["valid"].clone()
        valid[:, (seq - 1) // 64 * 64:] = False
        m["lse_without_last_tile"] = dict(lse=kr.attn_ref(
            q, k, v, dout, causal, scale, valid=valid)["lse"])
    return m


@pytest.fixture(scope="module")
def attn_mutation_ratios():
    """{mutation: {case label: worst err / (factor * E)}} over a slice of
    the GPU matrix"""
    res = {name: {} for name in ATTN_MUTATIONS}
    for family in kr.ATTN_FAMILIES:
        for seq, d in ((72, 64), (200, 64), (257, 128)):
            for causal in (False, True):
                for thresh, with_dlse in ((0, False), (128, True)):
                    case = _attn_case(family, seq, d, causal, thresh,
                                      with_dlse)
                    q, k, v, dout, scale, keep, inv_keep, dlse = case
                    ref = kr.attn_ref(q, k, v, dout, causal, scale, keep,
                                      inv_keep, dlse)
                    bounds = kr.attn_bounds(ref, q, k, v, dout, scale)
                    label = (family, seq, d, causal, thresh)
                    for name, outs in _attn_mutants(
                            *case[:4], causal, *case[4:], ref).items():
                        res[name][label] = max(
                            kr.attn_ratio((outs[o] - ref[o]).abs(),
                                          kr.ATTN_FACTOR[o] * bounds[o])
                            for o in ("out", "lse", "dq", "dk", "dv")
                            if o in outs)
    return res


@pytest.mark.parametrize("mutation", ATTN_MUTATIONS)
def test_attn_bounds_reject_mutation(attn_mutation_ratios, mutation):
    ratios = attn_mutation_ratios[mutation]
    assert ratios, mutation
    best = max(ratios, key=ratios.get)
    print(mutation, "worst err / allowed:", ratios[best], "at", best,
          "; weakest case:", min(ratios.values()))
    assert ratios[best] >= 10.0, (mutation, best, ratios[best])


def test_attn_layouts_and_unpack_keep():
    b, h, seq, d = kr.ATTN_B, kr.ATTN_H, 5, 64
    triplets = {}
    for name in kr.ATTN_LAYOUTS:
        lay = kr.attn_layout(name, b, h, seq, d, "cpu")
        for key in ("q", "k", "v", "out", "dout", "dq", "dk", "dv"):
            t = lay[key]
            assert t.shape == (b, h, seq, d) and t.stride(3) == 1
            assert t.stride(1) % 8 == 0 and t.stride(2) % 8 == 0
            assert t.storage_offset() % 8 == 0
            assert bool(torch.isnan(t.float()).all())    # sentinel
        assert lay["q"].stride() == lay["k"].stride() == lay["v"].stride()
        assert lay["dq"].stride() == lay["dk"].stride() == lay["dv"].stride()
        triplets[name] = [lay[key].stride()[:3]
                          for key in ("q", "out", "dout", "dq")]
        # a write through the views leaves the sentinels, one outside
        # them is noticed
        for key in ("out", "dq", "dk", "dv"):
            lay[key].fill_(1.0)
        assert all(buf.stray_writes() == 0
                   for buf in lay["buffers"].values())
        for buf in lay["buffers"].values():
            assert not bool(buf.addressed[:buf.guard].any())
            assert not bool(buf.addressed[-buf.guard:].any())
        victim = lay["buffers"]["out"]
        victim.raw[0] = 0
        assert victim.stray_writes() == 1
    assert len(set(triplets["padded"])) == 4
    assert lay["buffers"]["dq"].raw.numel() > b * h * seq * (d + 16)

    words = torch.tensor([0b101, -1, -2 ** 31, 0, 6, 7], dtype=torch.int32)
    keep = kr.unpack_keep(words, 2, 3)
    assert keep.tolist() == [[[1, 0, 1], [1, 1, 1], [0, 0, 0]],
                             [[0, 0, 0], [0, 1, 1], [1, 1, 1]]]
    gen = torch.Generator().manual_seed(3)
    bits = torch.randint(0, 2, (2, 40, 64), generator=gen)
    packed = (bits.reshape(2, 40, 2, 32) << torch.arange(32)).sum(-1)
    packed = torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed)
    keep = kr.unpack_keep(packed.to(torch.int32).reshape(-1), 2, 40)
    assert torch.equal(keep, bits[:, :, :40].to(F64))


# ---- LayerNorm, bias + GeLU, column sum -------------------------------------
def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(
        1.0, float(b.abs().max()))


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("rows,cols", [(1, 8), (37, 520), (37, 1000)])
def test_ln_ref_matches_torch(rows, cols, with_res):
    inp = kr.ln_inputs(rows, cols, with_res, dy_name="cancel")
    ref = kr.ln_ref(inp["x"], inp["res"], inp["gamma"], inp["beta"])
    s = inp["x"] if not with_res else inp["x"] + inp["res"]
    sa = s.clone().requires_grad_(True)
    ga = inp["gamma"].clone().requires_grad_(True)
    ba = inp["beta"].clone().requires_grad_(True)
    out = torch.nn.functional.layer_norm(sa, (cols,), ga, ba, kr.LN_EPS)
    assert _close(ref["out"], out.detach())
    assert _close(ref["mean"], s.mean(1))
    assert _close(ref["rstd"], (s.var(1, unbiased=False) + kr.LN_EPS) ** -0.5)
    out.backward(inp["dy"])
    bwd = kr.ln_bwd_ref(inp["dy"], s, inp["gamma"], ref["mean"],
                        ref["rstd"], inp["dadd"])
    # autograd's dx of a constant row is 0 * rstd: scale by the largest
    scale = max(1.0, float(sa.grad.abs().max()))
    assert float((bwd["dx_ln"] - sa.grad).abs().max()) <= 1e-12 * scale
    assert _close(bwd["dx"], sa.grad + inp["dadd"])
    assert _close(bwd["dgamma"], ga.grad)
    assert _close(bwd["dbeta"], ba.grad)
    assert _close(bwd["colsum"], (sa.grad + inp["dadd"]).sum(0))
    assert _close(kr.colsum_ref(inp["dy"]), inp["dy"].sum(0))


def test_bias_gelu_ref_matches_torch():
    inp = kr.bias_gelu_inputs(37, 520)
    ref = kr.bias_gelu_ref(inp["x"], inp["bias"], inp["dy"])
    xa = inp["x"].clone().requires_grad_(True)
    ba = inp["bias"].clone().requires_grad_(True)
    out = torch.nn.functional.gelu(xa + ba, approximate="tanh")
    out.backward(inp["dy"])
    assert _close(ref["out"], out.detach())
    assert _close(ref["dx"], xa.grad)
    assert _close(ref["dbias"], ba.grad)
    # the second derivative's bound used by bias_gelu_bounds
    z = torch.linspace(-14, 14, 280001, dtype=F64)
    g = kr.gelu_tanh_grad(z)
    d2 = (g[2:] - g[:-2]) / (z[2:] - z[:-2])
    assert 0.79 < float(d2.abs().max()) < kr.GELU_D2_MAX


def test_ln_and_gelu_inputs_have_their_properties():
    nk = len(kr.LN_KINDS)
    assert {f for _, f, _ in kr.LN_KINDS} == set(kr.LN_FAMILIES)
    for rows, cols in ((37, 1000), (37, 8), (3, 4096)):
        for with_res in (False, True):
            inp = kr.ln_inputs(rows, cols, with_res)
            for key in ("x", "gamma", "beta", "dy", "dadd"):
                assert torch.equal(kr.bf16_round(inp[key]), inp[key]), key
            again = kr.ln_inputs(rows, cols, with_res)
            assert torch.equal(inp["x"], again["x"])
            s = inp["x"]
            if with_res:
                assert torch.equal(kr.bf16_round(inp["res"]), inp["res"])
                s = s + inp["res"]
                assert float(inp["res"].abs().max()) > 0
            ref = kr.ln_ref(inp["x"], inp["res"], inp["gamma"], inp["beta"])
            assert float(inp["gamma"][cols // 3]) == 0
            assert float(inp["gamma"][cols - 1]) < 0
            for r in range(rows):
                name, family, par = kr.LN_KINDS[int(inp["kinds"][r])]
                row = s[r]
                if family != "randn":       # the sum is representable
                    assert torch.equal(kr.bf16_round(row), row), name
                if family == "const":
                    assert float(row.max()) == float(row.min())
                    assert abs(float(row[0]) - par) <= 2.0 ** -8 * abs(par)
                    assert float((ref["out"][r] - inp["beta"]).abs().max()) \
                        < 1e-9
                    assert abs(float(ref["rstd"][r]) * kr.LN_EPS ** 0.5 - 1) \
                        < 1e-12
                if family == "near_const":
                    base, step, m = par
                    m = max(1, min(m, cols // 2))
                    assert int((row == base).sum()) == cols - m
                    assert int((row == base + step).sum()) == m
                    assert float(kr.bf16_round(torch.tensor(
                        base + step / 2, dtype=F64))) in (base, base + step)
                if family == "offset":
                    assert abs(float(row.mean()) - par[1]) < par[0]
                if family == "tiny":
                    assert float(ref["var"][r]) < 1e-3 * kr.LN_EPS
                if family == "one_hot":
                    assert int((row != 0).sum()) == 1 and \
                        float(row.max()) == 1000.0
    for rows in (1, 3, 37):
        seen = set()
        for rot in kr.ln_rots(rows):
            seen |= set(kr.ln_row_kinds(rows, rot).tolist())
        assert seen == set(range(nk))
    gen = torch.Generator().manual_seed(0)
    co = kr.dy_family("coherent", 37, 24, gen)
    ca = kr.dy_family("cancel", 37, 24, gen)
    assert torch.equal(co.sum(0).abs(), co.abs().sum(0))
    assert torch.equal(ca[:36].sum(0), torch.zeros(24, dtype=F64))
    assert float(ca.abs().sum(0).min()) > 5
    # the GeLU sweep reaches both saturated ends and the derivative's
    # minimum, +-40 included, in every shape with room for it
    for rows, cols in ((1, 8), (3, 24), (37, 512), (1025, 1536)):
        inp = kr.bias_gelu_inputs(rows, cols)
        z = (inp["x"] + inp["bias"]).reshape(-1)[:inp["nsweep"]]
        assert torch.equal(kr.bf16_round(inp["x"]), inp["x"])
        assert float(z.max()) > 39 and float(z.min()) < -39
        if rows * cols >= 2 * kr.gelu_sweep().numel():
            assert float((z[:-2] - kr.gelu_sweep()[:-2]).abs().max()) < 0.07
            assert bool(((z > -0.8) & (z < -0.7)).any())
            assert float(z[:-2].min()) < -11.9 and float(z[:-2].max()) > 11.9


def _emu_fwd(bf16):
    return lambda inp, with_res: kr.ln_emulate(
        inp["x"], inp["res"], inp["gamma"], inp["beta"], bf16)


def _emu_bwd(bf16):
    def fn(inp, x_used, mean, rstd, dadd, want_colsum):
        return kr.ln_bwd_emulate(inp["dy"], x_used, inp["gamma"], mean, rstd,
                                 dadd, bf16)
    return fn


@pytest.mark.parametrize("cols,rows,bf16", kr.ln_cases())
def test_ln_emulation_inside_bounds(cols, rows, bf16):
    """the rounding model stays within the GPU tests' criterion on every
    element of every case of the GPU matrix: 1 x E on the fp32 results,
    2 x E on the bf16 tensors (E carries 2^-9 |ref| for the final
    rounding, and one correct bf16 rounding alone reaches 2^-8 |ref|).
    Every rstd bound is within 2^-12 relative, asserted by ln_check_case"""
    worst, bad = kr.ln_check_case(
        cols, rows, bf16, _emu_fwd(bf16), _emu_bwd(bf16),
        kr.LN_FACTOR_BF16 if bf16 else kr.LN_FACTOR_F32)
    print("LN-EMU cols %d rows %d bf16 %d %s"
          % (cols, rows, bf16, kr.format_worst(worst)))
    assert not bad, bad


@pytest.mark.parametrize("rows,cols,bf16", kr.gelu_cases())
def test_bias_gelu_emulation_inside_bounds(rows, cols, bf16):
    worst, bad = kr.gelu_check_case(
        rows, cols, bf16, lambda inp: kr.bias_gelu_emulate(
            inp["x"], inp["bias"], inp["dy"], bf16),
        kr.GELU_FACTOR_BF16 if bf16 else kr.GELU_FACTOR_F32)
    print("GELU-EMU rows %d cols %d bf16 %d %s"
          % (rows, cols, bf16, kr.format_worst(worst)))
    assert not bad, bad


@pytest.mark.parametrize("bf16", [True, False])
def test_colsum_emulation_inside_bounds(bf16):
    for cols in kr.COLSUM_COLS:
        for rows in kr.COLSUM_ROWS:
            for name in kr.LN_DY_FAMILIES:
                gen = torch.Generator().manual_seed(rows + cols)
                dy = kr.dy_family(name, rows, cols, gen)
                r = kr.ratio_of(kr.colsum_emulate(dy, bf16),
                                kr.colsum_ref(dy), kr.colsum_bounds(dy, bf16))
                assert r <= (2.0 if bf16 else 1.0), (cols, rows, name, r)


def test_two_moment_variance_breaks_the_listed_rows():
    """the parent kernels' var = sumsq / n - mean^2 in fp32 on the rows the
    issue lists: NaN or an rstd far outside the bound, where the shipped
    algorithm's emulation is inside it"""
    f = torch.float32
    for cols in (1000, 1536, 4096):
        inp = kr.ln_inputs(37, cols, False)
        ref = kr.ln_ref(inp["x"], None, inp["gamma"], inp["beta"])
        e = kr.ln_fwd_bounds(ref, inp["x"], None, inp["gamma"], inp["beta"],
                             True)
        x = inp["x"].to(f)
        mean = x.sum(1) / cols
        rstd = torch.rsqrt((x * x).sum(1) / cols - mean * mean + kr.LN_EPS)
        bad = ~((rstd.to(F64) - ref["rstd"]).abs() <= e["rstd"])
        kinds = {kr.LN_KINDS[int(k)][1] for k in inp["kinds"][bad]}
        assert {"offset", "near_const"} <= kinds, kinds
        emu = kr.ln_emulate(inp["x"], None, inp["gamma"], inp["beta"], True)
        assert bool(((emu["rstd"] - ref["rstd"]).abs() <= e["rstd"]).all())


LN_MUTATIONS = (
    "mean_of_neighbour_row", "rstd_without_eps", "two_moment_variance",
    "last_vector_outside_stats", "gamma_shifted_8", "beta_dropped",
    "residual_after_stats", "dx_without_sum_dygx", "dadd_dropped",
    "dgamma_missing_last_row", "dgamma_partial_twice", "colsum_before_dadd")


def _ln_mutants(inp, ref, bwd):
    """wrong kernels as mutated references: name -> {output: value}"""
    x, res, gamma, beta = inp["x"], inp["res"], inp["gamma"], inp["beta"]
    dy, dadd = inp["dy"], inp["dadd"]
    s, mean, rstd = ref["s"], ref["mean"], ref["rstd"]
    rows, cols = x.shape
    m = {}

    def out_at(mu, rs, g=gamma, b=beta):
        return (s - mu[:, None]) * rs[:, None] * g + b

    if rows > 1:
        mu = torch.roll(mean, 1)
        m["mean_of_neighbour_row"] = dict(mean=mu, out=out_at(mu, rstd))
    rs = ref["var"] ** -0.5
    m["rstd_without_eps"] = dict(rstd=rs, out=out_at(mean, rs))
    f = torch.float32
    s32 = s.to(f)
    mu32 = s32.sum(1) / cols
    rs32 = torch.rsqrt((s32 * s32).sum(1) / cols - mu32 * mu32 +
                       torch.tensor(kr.LN_EPS, dtype=f))
    m["two_moment_variance"] = dict(
        mean=mu32.to(F64), rstd=rs32.to(F64),
        out=out_at(mu32.to(F64), rs32.to(F64)))
    if cols > 8:
        part = kr.ln_ref(s[:, :-8], None, gamma[:-8], beta[:-8])
        m["last_vector_outside_stats"] = dict(
            mean=part["mean"], rstd=part["rstd"],
            out=out_at(part["mean"], part["rstd"]))
        m["gamma_shifted_8"] = dict(
            out=out_at(mean, rstd, g=torch.roll(gamma, 8)))
    m["beta_dropped"] = dict(out=out_at(mean, rstd, b=0 * beta))
    if res is not None:
        part = kr.ln_ref(x, None, gamma, beta)
        m["residual_after_stats"] = dict(
            mean=part["mean"], rstd=part["rstd"],
            out=out_at(part["mean"], part["rstd"]))
    m["dx_without_sum_dygx"] = dict(
        dx=(bwd["dyg"] - bwd["a"] / cols) * rstd[:, None] + dadd)
    m["dadd_dropped"] = dict(dx=bwd["dx_ln"], colsum=bwd["dx_ln"].sum(0))
    if rows > 1:
        m["dgamma_missing_last_row"] = dict(
            dgamma=bwd["dgamma"] - dy[-1] * bwd["xhat"][-1])
    own = slice(0, rows, kr.ln_bwd_waves(rows))     # the rows of wave 0
    m["dgamma_partial_twice"] = dict(
        dgamma=bwd["dgamma"] + (dy[own] * bwd["xhat"][own]).sum(0))
    m["colsum_before_dadd"] = dict(colsum=bwd["dx_ln"].sum(0))
    return m


@pytest.fixture(scope="module")
def ln_mutation_ratios():
    """{mutation: {case: worst err / (factor x E)}} over a slice of the
    matrix, backward at the reference statistics with dadd"""
    out = {name: {} for name in LN_MUTATIONS}
    for cols, rows in ((64, 3), (520, 37), (1536, 37), (4096, 37)):
        for with_res in (False, True):
            for dy_name in kr.LN_DY_FAMILIES:
                inp = kr.ln_inputs(rows, cols, with_res, dy_name)
                ref = kr.ln_ref(inp["x"], inp["res"], inp["gamma"],
                                inp["beta"])
                e = kr.ln_fwd_bounds(ref, inp["x"], inp["res"], inp["gamma"],
                                     inp["beta"], True)
                bwd = kr.ln_bwd_ref(inp["dy"], ref["s"], inp["gamma"],
                                    ref["mean"], ref["rstd"], inp["dadd"])
                e.update(kr.ln_bwd_bounds(
                    bwd, inp["dy"], ref["s"], inp["gamma"], ref["mean"],
                    ref["rstd"], inp["dadd"], True))
                want = dict(ref, **{k: bwd[k] for k in (
                    "dx", "dgamma", "dbeta", "colsum")})
                for name, outs in _ln_mutants(inp, ref, bwd).items():
                    out[name][(cols, rows, with_res, dy_name)] = max(
                        kr.ratio_of(v, want[o], kr.LN_FACTOR_BF16[o] * e[o])
                        for o, v in outs.items())
    return out


@pytest.mark.parametrize("mutation", LN_MUTATIONS)
def test_ln_bounds_reject_mutation(ln_mutation_ratios, mutation):
    ratios = ln_mutation_ratios[mutation]
    assert ratios, mutation
    best = max(ratios, key=ratios.get)
    print(mutation, "worst err / allowed:", ratios[best], "at", best,
          "; weakest case:", min(ratios.values()))
    assert ratios[best] >= 10.0, (mutation, best, ratios[best])


GELU_MUTATIONS = (
    "bias_of_neighbour_vector", "erf_gelu", "derivative_without_cubic",
    "dbias_segment_shifted", "dbias_missing_rows_from_1024")


@pytest.fixture(scope="module")
def gelu_mutation_ratios():
    out = {name: {} for name in GELU_MUTATIONS}
    for rows, cols in ((37, 24), (37, 1536), (1025, 1536)):
        inp = kr.bias_gelu_inputs(rows, cols)
        x, bias, dy = inp["x"], inp["bias"], inp["dy"]
        ref = kr.bias_gelu_ref(x, bias, dy)
        e = kr.bias_gelu_bounds(ref, x, bias, dy, True)
        z = ref["z"]
        mut = {}
        shifted = kr.bias_gelu_ref(x, torch.roll(bias, 8), dy)
        mut["bias_of_neighbour_vector"] = dict(
            out=shifted["out"], dx=shifted["dx"], dbias=shifted["dbias"])
        mut["erf_gelu"] = dict(out=torch.nn.functional.gelu(z))
        dx = dy * kr.gelu_tanh_grad(z, cubic=False)
        mut["derivative_without_cubic"] = dict(dx=dx, dbias=dx.sum(0))
        if cols >= 1024:
            mut["dbias_segment_shifted"] = dict(
                dbias=torch.roll(ref["dbias"], 512))
        if rows > 1024:
            mut["dbias_missing_rows_from_1024"] = dict(
                dbias=ref["dx"][:1024].sum(0))
        for name, outs in mut.items():
            out[name][(rows, cols)] = max(
                kr.ratio_of(v, ref[o], kr.GELU_FACTOR_BF16[o] * e[o])
                for o, v in outs.items())
    return out


@pytest.mark.parametrize("mutation", GELU_MUTATIONS)
def test_gelu_bounds_reject_mutation(gelu_mutation_ratios, mutation):
    ratios = gelu_mutation_ratios[mutation]
    assert ratios, mutation
    best = max(ratios, key=ratios.get)
    print(mutation, "worst err / allowed:", ratios[best], "at", best)
    assert ratios[best] >= 10.0, (mutation, best, ratios[best])
