"""Joint inputs, reference, rounding model, wrong kernels and case tables
for the grouped attention kernels (attention_gqa.hip, attention_band.hip,
attention_interval.hip).  Shared by test_attention_group_refs_cpu.py,
test_attention_group_edges_gpu.py and the three kernels' own GPU files (not
a test file).  Everything numeric comes from kernel_refs.py unchanged.

q has H heads, k and v have Hkv; query head h reads kv head h // G,
G = H // Hkv.  The families are built on q and k TOGETHER, so a steered row
meets the key it was steered onto and the shifted rows and keys share their
direction:

randn   : standard normal.
peaked  : q and k scaled by one factor so that max |s| is about 40, then
          the rows of kernel_refs.attn_peak_pairs steered onto their key
          of their own kv head, s = 40; under a mask a pair whose key the
          row cannot see moves to the nearest visible key.
shifted : a unit direction w per kv head, +-c w on the q rows of its G
          query heads and +c w on its keys, c^2 scale = 60.
edge    : needs the mask.  Rows steered (s = 40) onto their first and
          onto their last visible key, and lured rows: a HIDDEN key next
          to the row's visible interval at s = 40 while every visible
          score of the row stays O(1).  The reference never sees a lure; a
          kernel that lets one in is wrong by O(1), and one that loses a
          steered key too.  Lures live in coordinates of their own: the
          first L coordinates of q and k are zero but for lure t, which
          puts a on its key and beta on its row in coordinate t, so no
          other score moves.  Rows are chosen so that the steered or lured
          key sits at 31, 32, 33 (mod 64) and at 63, 64, 127, 128 wherever
          the mask has such a boundary; with lengths one lure sits on key
          len.  Entries are dealt over the query heads, one row of a head
          carries at most one.
"""

import functools
import math

import torch

from tests import kernel_refs as kr
from tests import varlen_refs as vr
from tests.test_attention_band_cpu import (CUTS_A, CUTS_B, band_valid,
                                           doc_ids)
from tests.test_attention_interval_cpu import interval_valid

F64 = torch.float64
FAMILIES = kr.ATTN_FAMILIES + ("edge",)
PEAK = 40.0
SHIFT = 60.0
EDGE_MOD64 = (31, 32, 33)
EDGE_KEYS = (63, 64, 127, 128)
STEERED = ("first", "last")
LURES = ("lure_lo", "lure_hi", "lure_key", "lure_len")


# ---------------------------------------------------------------------------
# masks as intervals
# ---------------------------------------------------------------------------
def intervals(mask):
    """(lo, hi) of every row of a [S, S] bool mask whose rows are the
    non-empty intervals [lo, hi)"""
    seq = mask.shape[-1]
    m = mask.to(torch.int8)
    lo = m.argmax(-1)
    hi = seq - m.flip(-1).argmax(-1)
    pos = torch.arange(seq)
    assert torch.equal(mask, (pos >= lo[:, None]) & (pos < hi[:, None]))
    return lo, hi


def is_causal(valid):
    seq = valid.shape[-1]
    above = torch.ones(seq, seq, dtype=torch.bool).triu(1)
    return not bool((valid & above).any())


def dense_valid(seq, b, causal, lens=None):
    """the [B, 1, S, S] mask of the GQA kernels: the brute-force masks of
    the band / interval tests with one document and no window"""
    lens = [seq] * b if lens is None else list(lens)
    return (band_valid if causal else interval_valid)(None, None, seq, lens)


def peak_pairs(valid, lens=None):
    """per sample the (row, key) pairs of the ``peaked`` family: those of
    kernel_refs.attn_peak_pairs at the sample's length, each key moved to
    the nearest key its row sees"""
    b, seq = valid.shape[0], valid.shape[-1]
    causal = is_causal(valid)
    res = []
    for n in range(b):
        ln = seq if lens is None else lens[n]
        pairs = []
        for row, key in (kr.attn_peak_pairs(ln, causal) if ln else ()):
            seen = valid[n, 0, row].nonzero().flatten()
            pairs.append((row, int(seen[(seen - key).abs().argmin()])))
        res.append(pairs)
    return res


# ---------------------------------------------------------------------------
# the edge plan
# ---------------------------------------------------------------------------
def edge_classes(key):
    """the boundary-offset classes a key belongs to"""
    return (["m%d" % m for m in EDGE_MOD64 if key % 64 == m] +
            ["k%d" % x for x in EDGE_KEYS if key == x])


def edge_slots(mask, ln):
    """{(kind, class): [(row, key), ..]}: every (row, key) a slot of the
    edge family could take in one sample.  Kinds: first / last (the row's
    first / last visible key), lure_lo / lure_hi (the hidden key before /
    after the row's interval), lure_key (the hidden query before / after a
    key's interval, where it is also next to that row's interval; only for
    a non-symmetric mask) and lure_len (key len).  Class "any" holds all
    of a kind.  Rows and interval ends are < len, lured keys < S."""
    seq = mask.shape[-1]
    slots = {}
    if ln == 0:
        return slots
    lo, hi = (t.tolist() for t in intervals(mask))

    def add(kind, row, key):
        for cls in ["any"] + edge_classes(key):
            slots.setdefault((kind, cls), []).append((row, key))

    for i in range(ln):
        add("first", i, lo[i])
        add("last", i, hi[i] - 1)
        if lo[i] > 0:
            add("lure_lo", i, lo[i] - 1)
        if hi[i] < seq:
            add("lure_hi", i, hi[i])
            if hi[i] == ln:
                slots.setdefault(("lure_len", "len"), []).append((i, ln))
    if not torch.equal(mask[:ln, :ln], mask[:ln, :ln].T):
        qlo, qhi = (t.tolist() for t in intervals(mask.T))
        for j in range(seq):
            for i in (qlo[j] - 1, qhi[j]):
                if 0 <= i < ln and not mask[i, j] and j in (lo[i] - 1, hi[i]):
                    add("lure_key", i, j)
    return slots


def edge_plan(valid, h, lens=None):
    """per sample [(head, row, key, kind, class)]: one entry per slot of
    edge_slots, scarcest slot first, dealt over the query heads, on a
    (head, row) no other entry uses.  Also returns the slots."""
    b, seq = valid.shape[0], valid.shape[-1]
    plans, all_slots = [], []
    for n in range(b):
        ln = seq if lens is None else lens[n]
        slots = edge_slots(valid[n, 0], ln)
        used, plan = set(), []
        order = sorted(slots.items(), key=lambda kv: (len(kv[1]), kv[0]))
        for t, ((kind, cls), cands) in enumerate(order):
            mid = len(cands) // 2
            for head in ((t + dh) % h for dh in range(h)):
                free = [c for c in cands[mid:] + cands[:mid]
                        if (head, c[0]) not in used]
                if free:
                    row, key = free[0]
                    used.add((head, row))
                    plan.append((head, row, key, kind, cls))
                    break
        plans.append(plan)
        all_slots.append(slots)
    return plans, all_slots


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def _steer(q, k, n, head, g, row, key, scale):
    kj = k[n, head // g, key]
    q[n, head, row] = kj * (PEAK / (scale * float((kj * kj).sum())))


def group_build(family, seq, d, h, hkv, b, valid=None, seed=0, lens=None):
    """(q, k, v, dout, info) of the module docstring: fp64 tensors of
    bf16-representable values, q / dout [b,h,S,d], k / v [b,hkv,S,d].
    valid: the brute-force [b,1,S,S] mask (None: dense non-causal); lens:
    the per-sample lengths that mask was built with.  info names what was
    steered: ``pairs`` (per sample (head or None, row, key)), ``lures``
    (the same), ``w`` and ``c`` of ``shifted``, ``plan`` / ``slots`` of
    ``edge``."""
    assert family in FAMILIES and h % hkv == 0
    g = h // hkv
    gen = torch.Generator().manual_seed(
        seed + 1000 * FAMILIES.index(family) + 7 * seq + d + 31 * h +
        131 * hkv + 977 * b)
    scale = 1.0 / math.sqrt(d)
    q, dout = (torch.randn(b, h, seq, d, generator=gen, dtype=F64)
               for _ in range(2))
    k, v = (torch.randn(b, hkv, seq, d, generator=gen, dtype=F64)
            for _ in range(2))
    info = dict(pairs=[[] for _ in range(b)], lures=[[] for _ in range(b)])
    if valid is None:
        assert family != "edge", "edge needs the mask"
        valid = dense_valid(seq, b, False, lens)
    assert valid.shape == (b, 1, seq, seq)
    if family == "peaked":
        ke = k.repeat_interleave(g, dim=1)
        smax = (torch.matmul(q, ke.transpose(-1, -2)) * scale).abs().max()
        f = math.sqrt(PEAK / smax.item())
        q, k = q * f, kr.bf16_round(k * f)
        for n, pairs in enumerate(peak_pairs(valid, lens)):
            for row, key in pairs:
                for head in range(h):
                    _steer(q, k, n, head, g, row, key, scale)
                info["pairs"][n].append((None, row, key))
    elif family == "shifted":
        w = torch.randn(b, hkv, 1, d, generator=gen, dtype=F64)
        w = w / w.norm(dim=-1, keepdim=True)
        c = math.sqrt(SHIFT / scale)
        sign = torch.where((torch.arange(seq) // 2) % 2 == 0, 1.0, -1.0)
        q = q + c * sign.to(F64)[None, None, :, None] * \
            w.repeat_interleave(g, dim=1)
        k = k + c * w
        info.update(w=w, c=c, sign=sign)
    elif family == "edge":
        q, k = kr.bf16_round(q), kr.bf16_round(k)
        plans, slots = edge_plan(valid, h, lens)
        info.update(plan=plans, slots=slots)
        a = float(kr.bf16_round(torch.tensor(math.sqrt(PEAK / scale),
                                             dtype=F64)))
        for n, plan in enumerate(plans):
            lures = [e for e in plan if e[3] in LURES]
            count = [0] * hkv
            axis = {}
            for e in lures:
                axis[e[:2]] = count[e[0] // g]
                count[e[0] // g] += 1
            width = max(count)
            assert width <= d // 2, (width, d)
            q[n, :, :, :width] = 0.0
            k[n, :, :, :width] = 0.0
            for head, row, key, _, _ in lures:
                k[n, head // g, key, axis[(head, row)]] = a
            for head, row, key, _, _ in lures:
                rest = float((q[n, head, row] * k[n, head // g, key]).sum())
                q[n, head, row, axis[(head, row)]] = (PEAK / scale - rest) / a
                info["lures"][n].append((head, row, key))
            for head, row, key, kind, _ in plan:
                if kind in STEERED:
                    _steer(q, k, n, head, g, row, key, scale)
                    info["pairs"][n].append((head, row, key))
    q, k, v, dout = (kr.bf16_round(t) for t in (q, k, v, dout))
    return q, k, v, dout, info


def group_inputs(family, seq, d, h, hkv, b, valid=None, seed=0, lens=None):
    return group_build(family, seq, d, h, hkv, b, valid, seed, lens)[:4]


# ---------------------------------------------------------------------------
# reference, rounding model, criterion
# ---------------------------------------------------------------------------
def _group_sum(t, hkv):
    b, h, seq, d = t.shape
    return t.view(b, hkv, h // hkv, seq, d).sum(2)


def group_reference(q, k, v, dout, valid):
    """(ref, bounds): attn_ref / attn_bounds on k and v expanded with
    repeat_interleave, dk / dv and their bounds summed over each group (the
    kernels add a group's fp32 contributions and round once; the triangle
    inequality).  valid: [B or 1, 1, S, S].  delta is judged by
    group_ratios on the kernel's own out."""
    h, d, hkv = q.shape[1], q.shape[3], k.shape[1]
    ke, ve = (t.repeat_interleave(h // hkv, dim=1) for t in (k, v))
    ref = kr.attn_ref(q, ke, ve, dout, False, d ** -0.5, valid=valid)
    bounds = kr.attn_bounds(ref, q, ke, ve, dout, d ** -0.5)
    for name in ("dk", "dv"):
        ref[name] = _group_sum(ref[name], hkv)
        bounds[name] = _group_sum(bounds[name], hkv)
    return ref, bounds


def group_emulate(q, k, v, dout, valid):
    """varlen_refs._emulate (the kernels' bf16 roundings under a mask) on
    the expanded k and v, dk / dv summed per group"""
    h, d, hkv = q.shape[1], q.shape[3], k.shape[1]
    ke, ve = (t.repeat_interleave(h // hkv, dim=1) for t in (k, v))
    emu = vr._emulate(q, ke, ve, dout, d ** -0.5, None, 1.0, None, valid)
    for name in ("dk", "dv"):
        emu[name] = _group_sum(emu[name], hkv)
    return emu


def group_ratios(got, ref, bounds, dout, lens=None, names=kr.ATTN_OUTPUTS):
    """worst err / E per output over the rows < len of every sample; delta
    against attn_delta_ref on ``got``'s own out"""
    res = {}
    for name in names:
        want, bound = ref[name], bounds[name]
        if name == "delta":
            want, bound = kr.attn_delta_ref(dout, got["out"])
        worst = 0.0
        for n in range(got[name].shape[0]):
            ln = got[name].shape[2] if lens is None else lens[n]
            if ln == 0:
                continue
            worst = max(worst, kr.attn_ratio(
                (got[name][n, :, :ln] - want[n, :, :ln]).abs(),
                bound[n, :, :ln]))
        res[name] = worst
    return res


# ---------------------------------------------------------------------------
# wrong kernels
# ---------------------------------------------------------------------------
def staged_model(q, k, v, dout, valid, dq_valid=None, kv_valid=None,
                 head_map="interleave", drop_last_head=False):
    """The kernels by stage, in fp64: the forward (out, lse, delta) under
    ``valid``, the dQ kernel under ``dq_valid`` and the dK/dV kernel under
    ``kv_valid`` (both default to ``valid``), each taking P = exp(s - lse)
    from the forward's lse as the kernels do.  head_map "modulo" reads kv
    head h % Hkv; drop_last_head leaves each group's last query head out of
    dk / dv.  With the defaults this is group_reference's ref."""
    b, h, seq, d = q.shape
    hkv = k.shape[1]
    g = h // hkv
    idx = torch.arange(h) // g if head_map == "interleave" \
        else torch.arange(h) % hkv
    ke, ve = k[:, idx], v[:, idx]
    scale = d ** -0.5
    s = torch.matmul(q, ke.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s.masked_fill(~valid, float("-inf")), dim=-1)
    e = torch.exp(s - lse.unsqueeze(-1))
    out = torch.matmul(e.masked_fill(~valid, 0.0), ve)
    delta = (dout * out).sum(dim=-1)
    dp = torch.matmul(dout, ve.transpose(-1, -2))

    def stage(mask):
        p = e.masked_fill(~(valid if mask is None else mask), 0.0)
        return p, p * (dp - delta.unsqueeze(-1)) * scale

    _, ds = stage(dq_valid)
    dq = torch.matmul(ds, ke)
    p, ds = stage(kv_valid)
    keep = torch.ones(h, dtype=F64)
    if drop_last_head:
        keep[g - 1::g] = 0.0
    keep = keep[None, :, None, None]
    dk, dv = (torch.zeros(b, hkv, seq, d, dtype=F64).index_add_(1, idx, t)
              for t in (torch.matmul(ds.transpose(-1, -2), q) * keep,
                        torch.matmul(p.transpose(-1, -2), dout) * keep))
    return dict(out=out, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)


def moved_mask(valid, side, step, lens=None, only32=False, keys=False):
    """``valid`` with one bound of every interval moved by ``step``:
    side "lo" or "hi" of the rows' intervals (kv_lo / kv_hi), or with
    ``keys`` of the keys' intervals (q_lo / q_hi).  only32: just the rows
    (keys) whose bound is a multiple of 32.  Intervals stay non-empty and
    inside [0, len); rows (keys) >= len stay as they are."""
    b, seq = valid.shape[0], valid.shape[-1]
    res = valid.clone()
    pos = torch.arange(seq)
    for n in range(b):
        ln = seq if lens is None else lens[n]
        if ln == 0:
            continue
        m = valid[n, 0].T if keys else valid[n, 0]
        lo, hi = intervals(m)
        bound = lo if side == "lo" else hi
        pick = (pos < ln) & ((bound % 32 == 0) if only32 else True)
        new = torch.where(pick, bound + step, bound)
        if side == "lo":
            lo = new.clamp(min=0).minimum(hi - 1)
        else:
            hi = torch.where(pos < ln, new.clamp(max=ln), hi).maximum(lo + 1)
        m = (pos >= lo[:, None]) & (pos < hi[:, None])
        res[n, 0] = m.T if keys else m
    return res


# ---------------------------------------------------------------------------
# the cases of test_attention_group_edges_gpu.py
# ---------------------------------------------------------------------------
B = 2
DIMS = (64, 128)
HEADS = ((4, 4), (4, 1), (8, 2))
KERNELS = ("gqa", "gqa_causal", "band", "interval")
DOCS_A, DOCS_B = (1, 32, 64, 128), (31, 33, 65)
PREFIX = (33, 128)
# name -> (seq, document cuts per sample or None, window, lengths)
CASES = {
    "s1": (1, None, None, None),
    "s31": (31, None, None, None),
    "s33": (33, None, None, None),
    "s64": (64, None, None, None),
    "s65": (65, None, None, None),
    "s129": (129, None, None, None),
    "docs129": (129, (DOCS_A, DOCS_B), None, None),
    "win1": (200, ((), (97,)), 1, None),
    "win32": (200, ((), (97,)), 32, None),
    "win33": (200, ((), (97,)), 33, None),
    "win64": (200, ((), (97,)), 64, None),
    "win65": (200, ((), (97,)), 65, None),
    "docs_win40_lens": (257, (CUTS_A, CUTS_B), 40, (257, 130)),
    "lens01": (200, None, None, (0, 1)),
    "prefix_lm": (200, None, None, None),
}
SHORT = ("s1", "s31", "s33", "s64", "s65", "s129")
KERNEL_CASES = {
    "gqa": SHORT + ("lens01",),
    "gqa_causal": SHORT + ("lens01",),
    "band": tuple(c for c in CASES if c != "prefix_lm"),
    "interval": tuple(CASES),
}
MAIN = [(kernel, d, h, hkv, case) for kernel in KERNELS for d in DIMS
        for h, hkv in HEADS for case in KERNEL_CASES[kernel]]
# block order: 9 and 17 batch-kv-heads, every sample bounded differently
ORDER_DOCS = ((1, 33, 128, 200), (31, 32, 64, 129), (65, 127, 256))
ORDER_LENS = (257, 130, 65)
ORDER = [(kernel, 3, 6, 3) for kernel in KERNELS] + \
    [(kernel, 17, 2, 1) for kernel in ("band", "interval")]


def main_family(index):
    return FAMILIES[index % len(FAMILIES)]


def main_layout(index):
    return ("plain", "padded")[(index // len(FAMILIES)) % 2]


def prefix_bounds(seq, prefix=PREFIX):
    """(kv_lo, kv_hi, q_lo, q_hi), int64 [B, S], of prefix-LM samples"""
    pos = torch.arange(seq)
    p = torch.tensor(prefix)[:, None]
    kv_hi = torch.maximum(pos + 1, p)
    return (torch.zeros_like(kv_hi), kv_hi, torch.where(pos < p, 0, pos),
            torch.full_like(kv_hi, seq))


def prefix_valid(seq, prefix=PREFIX):
    """[B, 1, S, S] by the definition: key j is seen by query i iff j <= i
    or j < p"""
    i, j = torch.arange(seq)[:, None], torch.arange(seq)[None, :]
    return torch.stack([((j <= i) | (j < p))[None] for p in prefix])


def order_cuts(kernel, b):
    if b == len(ORDER_DOCS):
        return ORDER_DOCS
    return tuple((1 + 7 * n, 64 + 3 * n, 128 + n) for n in range(b))


@functools.lru_cache(maxsize=None)
def case_mask(kernel, case, b=B):
    """(seq, ids or None, window, lens or None, [b,1,S,S] mask) of a case
    under a kernel: causal for gqa_causal and band.  Cached and shared:
    nobody writes into the mask."""
    causal = kernel in ("gqa_causal", "band")
    if case == "order":
        seq, window = 257, None
        if kernel in ("gqa", "gqa_causal"):
            ids, lens = None, ORDER_LENS
        else:
            ids = torch.stack([doc_ids(seq, c) for c in order_cuts(kernel, b)])
            lens = None
    else:
        seq, cuts, window, lens = CASES[case]
        ids = None if cuts is None else torch.stack(
            [doc_ids(seq, c) for c in cuts])
    if case == "prefix_lm":
        assert kernel == "interval"
        return seq, None, None, None, prefix_valid(seq)
    assert kernel in ("band", "interval") or (ids is None and window is None)
    brute = band_valid if causal else interval_valid
    return seq, ids, window, lens, brute(ids, window, seq,
                                         list(lens or [seq] * b))
