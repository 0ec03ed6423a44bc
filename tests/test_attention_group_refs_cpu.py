"""attn_group_cases.py checked without a GPU: the joint input families are
what they claim on every case the GPU files run, the kernels' rounding
model stays within 1 x E of the reference on every case of
test_attention_group_edges_gpu.py, and wrong kernels, written as mutations
of the reference, each exceed the allowed error at least tenfold on an
output that only the mutated kernel writes."""

import pytest
import torch

from tests import attn_group_cases as gc
from tests import kernel_refs as kr

F64 = torch.float64
U = kr.U_BF16        # one bf16 rounding of a q element


def test_rotation_meets_every_kernel_dim_and_group():
    seen = {(gc.main_family(i), key)
            for i, (kernel, d, h, hkv, _) in enumerate(gc.MAIN)
            for key in (("kernel", kernel), ("d", d), ("g", h // hkv))}
    for family in gc.FAMILIES:
        for key in [("kernel", k) for k in gc.KERNELS] + \
                [("d", d) for d in gc.DIMS] + \
                [("g", h // hkv) for h, hkv in gc.HEADS]:
            assert (family, key) in seen, (family, key)
    assert {gc.main_layout(i) for i in range(len(gc.MAIN))} == \
        {"plain", "padded"}


def _score(q, k, n, head, g, row, key, scale):
    prod = q[n, head, row] * k[n, head // g, key]
    return float(prod.sum()) * scale, float(prod.abs().sum()) * scale


def check_claims(family, built, valid, lens, label):
    """the properties of section B.1 for one built input"""
    q, k, v, dout, info = built
    b, h, seq, d = q.shape
    g = h // k.shape[1]
    scale = d ** -0.5
    for t in (q, k, v, dout):
        assert torch.equal(kr.bf16_round(t), t)
    steered = 0
    for n in range(b):
        ln = seq if lens is None else lens[n]
        for head, row, key in info["pairs"][n]:
            for hd in (range(h) if head is None else (head,)):
                s, mag = _score(q, k, n, hd, g, row, key, scale)
                assert row < ln and bool(valid[n, 0, row, key]), label
                assert abs(s - gc.PEAK) <= U * mag + 1e-9, (label, s)
                steered += 1
    if family == "peaked":
        assert steered or all(x == 0 for x in (lens or [1])), label
    if family == "shifted":
        wq = info["w"].repeat_interleave(g, dim=1)
        offset = scale * info["c"] * (q * wq).sum(-1)
        assert bool(((offset.abs() >= 45) & (offset.abs() <= 75)).all()), (
            label, float(offset.abs().min()), float(offset.abs().max()))
        assert bool((offset.sign() == info["sign"]).all()), label
    if family != "edge":
        return {}
    ke = k.repeat_interleave(g, dim=1)
    for n in range(b):
        ln = seq if lens is None else lens[n]
        lo, hi = gc.intervals(valid[n, 0])
        for head, row, key in info["lures"][n]:
            s, mag = _score(q, k, n, head, g, row, key, scale)
            assert row < ln and not bool(valid[n, 0, row, key]), label
            assert key in (int(lo[row]) - 1, int(hi[row])), label
            assert abs(s - gc.PEAK) <= U * mag + 1e-9, (label, s)
            seen = (ke[n, head] @ q[n, head, row]) * scale
            assert s - float(seen[valid[n, 0, row]].max()) >= 30.0, label
        placed = {(kind, cls) for _, _, _, kind, cls in info["plan"][n]}
        assert placed == set(info["slots"][n]), (
            label, n, set(info["slots"][n]) - placed)
    # how many entries of each boundary class this input carries
    count = {}
    for plan in info["plan"]:
        for _, _, _, kind, cls in plan:
            count[(kind, cls)] = count.get((kind, cls), 0) + 1
    return count


def test_families_on_the_edges_matrix():
    """every case of the GPU matrix with the family it runs there, and all
    four families at d 64, (H, Hkv) = (8, 2)"""
    classes = {}
    for index, (kernel, d, h, hkv, case) in enumerate(gc.MAIN):
        seq, _, _, lens, valid = gc.case_mask(kernel, case)
        families = {gc.main_family(index)}
        if (d, h) == (64, 8):
            families = set(gc.FAMILIES)
        for family in sorted(families):
            built = gc.group_build(family, seq, d, h, hkv, gc.B, valid,
                                   lens=lens)
            count = check_claims(family, built, valid, lens,
                                 (kernel, d, h, hkv, case, family))
            for key in count:
                classes.setdefault((kernel, case), set()).add(key)
    # a window, a document edge or a diagonal crossing 31 .. 33 and
    # 63 / 64 / 127 / 128 carries every class of every kind it has
    kinds = {"band": ("first", "last", "lure_lo", "lure_hi"),
             "interval": ("first", "last", "lure_lo", "lure_hi")}
    every = ["m%d" % m for m in gc.EDGE_MOD64] + \
        ["k%d" % x for x in gc.EDGE_KEYS]
    for kernel in kinds:
        for case in ("win33",):
            for kind in kinds[kernel]:
                for cls in every:
                    assert (kind, cls) in classes[(kernel, case)], (
                        kernel, case, kind, cls)
    assert ("lure_len", "len") in classes[("band", "docs_win40_lens")]
    assert ("lure_len", "len") in classes[("interval", "docs_win40_lens")]
    assert ("lure_len", "len") in classes[("gqa_causal", "lens01")]
    assert any(kind == "lure_key" for kind, _ in
               classes[("interval", "prefix_lm")])


def test_families_on_the_block_order_cases():
    for kernel, b, h, hkv in gc.ORDER:
        seq, _, _, lens, valid = gc.case_mask(kernel, "order", b)
        built = gc.group_build("peaked", seq, 64, h, hkv, b, valid,
                               lens=lens)
        check_claims("peaked", built, valid, lens, (kernel, b))
        masks = {valid[n].numpy().tobytes() for n in range(b)}
        assert len(masks) == b, "every sample bounded differently"


def test_families_on_the_three_kernel_files():
    """the case lists of test_attention_gqa_gpu.py,
    test_attention_band_gpu.py and test_attention_interval_gpu.py"""
    from tests import test_attention_band_gpu as band
    from tests import test_attention_gqa_gpu as gqa
    from tests import test_attention_interval_gpu as interval
    d = 64
    for name in band.BANDS:
        seq, ids, window, lens = band.band_of(name)
        valid = gc.band_valid(ids, window, seq, lens or [seq] * band.B)
        for family in kr.ATTN_FAMILIES:
            built = gc.group_build(family, seq, d, 4, 2, band.B, valid,
                                   lens=lens)
            check_claims(family, built, valid, lens, ("band", name, family))
    for name in interval.CASES:
        seq, lens, valid = interval.mask_of(name)
        for family in kr.ATTN_FAMILIES:
            built = gc.group_build(family, seq, d, 4, 2, interval.B, valid,
                                   lens=lens)
            check_claims(family, built, valid, lens,
                         ("interval", name, family))
    for seq, family in gqa.CASES + [(200, "shifted")]:
        for causal in (False, True):
            for hkv in (3, 2, 1):
                valid = gc.dense_valid(seq, 2, causal)
                built = gc.group_build(family, seq, d, 6, hkv, 2, valid)
                check_claims(family, built, valid, None,
                             ("gqa", seq, causal, hkv, family))


# ---------------------------------------------------------------------------
# the rounding model
# ---------------------------------------------------------------------------
def _model_ratios(kernel, d, h, hkv, case, family, b=gc.B):
    seq, _, _, lens, valid = gc.case_mask(kernel, case, b)
    inp = gc.group_inputs(family, seq, d, h, hkv, b, valid, lens=lens)
    ref, bounds = gc.group_reference(*inp, valid)
    emu = gc.group_emulate(*inp, valid)
    return gc.group_ratios(emu, ref, bounds, inp[3], lens)


@pytest.mark.parametrize("kernel", gc.KERNELS)
def test_model_inside_bounds_on_the_edges_matrix(kernel):
    worst = {}
    for index, (kern, d, h, hkv, case) in enumerate(gc.MAIN):
        if kern != kernel:
            continue
        family = gc.main_family(index)
        for name, r in _model_ratios(kern, d, h, hkv, case, family).items():
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, (kern, d, h, hkv, case, family, name, r)
    print("GROUP-MODEL", kernel, " ".join(
        "{}={:.3f}".format(n, worst[n]) for n in kr.ATTN_OUTPUTS))


def test_model_inside_bounds_on_the_block_order_cases():
    worst = {}
    for kernel, b, h, hkv in gc.ORDER:
        for name, r in _model_ratios(kernel, 64, h, hkv, "order", "peaked",
                                     b).items():
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, (kernel, b, name, r)
    print("GROUP-MODEL order", " ".join(
        "{}={:.3f}".format(n, worst[n]) for n in kr.ATTN_OUTPUTS))


# ---------------------------------------------------------------------------
# wrong kernels
# ---------------------------------------------------------------------------
FWD, DQ, KV = ("out", "lse"), ("dq",), ("dk", "dv")
EVERY = FWD + DQ + KV
MUTANT_CASES = {"band": ("docs129", "win33", "docs_win40_lens"),
                "interval": ("docs129", "win33", "docs_win40_lens",
                             "prefix_lm")}
MOVES = (("lo", -1), ("lo", 1), ("hi", 1), ("hi", -1))


def _mutants(inp, valid, lens, case):
    """name -> (outputs of a wrong kernel, the outputs it is judged on)"""
    def model(**kw):
        return gc.staged_model(*inp, **kw)

    res = {}
    for only32 in (False, True):
        tag = "@32" if only32 else ""
        for side, step in MOVES:
            rows = gc.moved_mask(valid, side, step, lens, only32)
            keys = gc.moved_mask(valid, side, step, lens, only32, keys=True)
            res["fwd kv_{}{:+d}{}".format(side, step, tag)] = (
                model(valid=rows, dq_valid=valid, kv_valid=valid), FWD)
            res["dq kv_{}{:+d}{}".format(side, step, tag)] = (
                model(valid=valid, dq_valid=rows), DQ)
            res["dkdv q_{}{:+d}{}".format(side, step, tag)] = (
                model(valid=valid, kv_valid=keys), KV)
    res["kv head h % Hkv"] = (model(valid=valid, head_map="modulo"), EVERY)
    res["last head of the group missing"] = (
        model(valid=valid, drop_last_head=True), KV)
    if not torch.equal(valid[0], valid[1]):
        swapped = valid.clone()
        swapped[1] = valid[0]
        res["sample 0's bounds on sample 1"] = (model(valid=swapped), EVERY)
    if lens is not None:
        loose = valid.clone()
        for n, ln in enumerate(lens):
            if 0 < ln < valid.shape[-1]:
                _, hi = gc.intervals(valid[n, 0])
                loose[n, 0, :ln, ln] = hi[:ln] == ln
        res["kv_hi not clamped to len"] = (model(valid=loose), FWD + DQ)
    if case == "prefix_lm":
        _, _, q_lo, _ = gc.prefix_bounds(valid.shape[-1])
        pos = torch.arange(valid.shape[-1])
        wrong = valid & (pos[None, None, :] >= q_lo[:, :, None])[:, None]
        res["prefix-LM: q_lo for kv_lo"] = (
            model(valid=wrong, kv_valid=valid), FWD + DQ)
    return res


@pytest.fixture(scope="module")
def mutation_ratios():
    """{kernel: {mutant: {family: worst err / allowed over the cases}}}"""
    d, h, hkv = 64, 4, 2
    res = {}
    for kernel, cases in MUTANT_CASES.items():
        table = res.setdefault(kernel, {})
        for case in cases:
            seq, _, _, lens, valid = gc.case_mask(kernel, case)
            for family in gc.FAMILIES:
                inp = gc.group_inputs(family, seq, d, h, hkv, gc.B, valid,
                                      lens=lens)
                ref, bounds = gc.group_reference(*inp, valid)
                good = gc.group_ratios(gc.staged_model(*inp, valid=valid),
                                       ref, bounds, inp[3], lens)
                assert max(good.values()) <= 1e-6, (kernel, case, good)
                for name, (outs, judged) in _mutants(inp, valid, lens,
                                                     case).items():
                    ratios = gc.group_ratios(outs, ref, bounds, inp[3],
                                             lens, judged)
                    r = max(ratios[o] / kr.ATTN_FACTOR[o] for o in judged)
                    row = table.setdefault(name, {})
                    row[family] = max(row.get(family, 0.0), r)
    return res


@pytest.mark.parametrize("kernel", list(MUTANT_CASES))
def test_criterion_rejects_the_wrong_kernels(mutation_ratios, kernel):
    table = mutation_ratios[kernel]
    assert len(table) >= 24 + 4
    for name, row in table.items():
        best = max(row, key=row.get)
        print("GROUP-MUTANT {} | {} | {} | {}".format(
            kernel, name, best, " ".join("{}={:.3g}".format(f, row[f])
                                         for f in gc.FAMILIES)))
    for name, row in table.items():
        assert max(row.values()) >= 10.0, (kernel, name, row)
        # the boundary mutants are what ``edge`` is for
        if name.split()[0] in ("fwd", "dq", "dkdv"):
            assert row["edge"] >= 10.0, (kernel, name, row)
