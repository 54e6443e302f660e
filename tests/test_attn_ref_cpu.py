"""The paged attention model and bound of tests/attn_ref.py cannot hide a wrong kernel (CPU only).

emulate() is a plain float32 / bf16 restatement of attn_rows_body's tile loop in torch -- the online softmax in tiles
of kt keys, the three bf16 products (exact products accumulated in float64 and rounded to float32 once a tile), static
or ticketed splits merged with k_attn_combine's arithmetic -- a test helper, never a reference.  Unmutated it must
stay at or below the bound E on every family, and each of its mutants (a wrong kernel) must exceed E on its named
family at head sizes 32, 64 and 128.  The exactness properties and the input conditions of attn_ref's docstring are
asserted for every case of its tables, the GPU test's included.
"""
import math

import numpy as np
import pytest
import torch

import attn_ref as ar

INF = math.inf
MUTANTS = {   # mutant -> the family that must expose it
    "drop_qh_kl": "lo_k", "drop_ql_kh": "lo_q", "drop_ph_vl": "lo_v", "drop_pl_vh": "lo_p",
    "no_alpha": "ascend",               # the accumulator is not rescaled when the maximum rises
    "stale_max": "descend",             # p is taken against the tile's own maximum
    "mask+1": "ascend",                 # the extra key is the next token's: the highest score of an ascend row
    "mask-1": "own",
    "merge_no_skip_nan": "flat",        # an empty split's (-inf, 0) partial is given weight: 0 times its unwritten o
    "merge_max_of_empty": "descend",    # an empty split publishes (0, 0) and M is taken over every split
    "tile_edge": "own",                 # the last key of a tile is dropped
    "row_swap": "own",                  # token 1's rows mask with token 0's key count
}


def exp32(x):
    return torch.exp(x.float())


def split(x):
    hi = x.float().bfloat16().float()
    return hi.double(), (x.float() - hi).bfloat16().float().double()


def emulate(q, K, V, nvis, H, KVH, kt, nsplit, kps, mut=()):
    """-> out [tn][H hd] float32"""
    tn, hd = q.shape[0], q.shape[2]
    G = H // KVH
    nv = torch.tensor(nvis)
    if "row_swap" in mut and tn > 1:
        nv[1] = nv[0]
    nv = nv + (1 if "mask+1" in mut else -1 if "mask-1" in mut else 0)
    nv = nv.repeat_interleave(G)
    Lmax = max(nvis)
    ns = ar.split_count(Lmax, nsplit, kps)
    per = ar.split_len(Lmax, ns, kt)
    out = torch.empty(tn, H, hd, dtype=torch.float32)
    for kh in range(KVH):
        qh, ql = split(q[:, kh * G:(kh + 1) * G].reshape(tn * G, hd) * np.float32(ar.SCALE))
        (kh_, kl), (vh, vl) = split(K[:, kh]), split(V[:, kh])
        R = qh.shape[0]
        parts = []
        for sp in range(ns):
            c0, c1 = sp * per, min(Lmax, sp * per + per)
            if c0 >= c1:    # the neutral partial; part_o stays as the launch found it (NaN under the poison protocol)
                parts.append((torch.full((R,), 0.0 if "merge_max_of_empty" in mut else -INF), torch.zeros(R),
                              torch.full((R, hd), math.nan), True))
                continue
            m, l, acc = torch.full((R,), -INF), torch.zeros(R), torch.zeros(R, hd)
            for k0 in range(c0, c1, kt):
                keys = torch.arange(k0, k0 + kt)
                kc = keys.clamp(max=c1 - 1)
                s = qh @ kh_[kc].t()
                if "drop_qh_kl" not in mut:
                    s = s + qh @ kl[kc].t()
                if "drop_ql_kh" not in mut:
                    s = s + ql @ kh_[kc].t()
                s = s.float()
                valid = (keys[None] < c1) & (keys[None] < nv[:, None])
                if "tile_edge" in mut:
                    valid = valid & ((keys - k0) != kt - 1)[None]
                tm = s.masked_fill(~valid, -INF).max(-1).values
                mn = torch.maximum(m, tm)
                alpha = torch.where(m == mn, torch.ones(R), exp32(m - mn))
                pm = tm if "stale_max" in mut else mn
                p = torch.where(valid, exp32(s - pm[:, None]), torch.zeros(()))
                l = ((l * alpha).double() + p.double().sum(-1)).float()
                if "no_alpha" not in mut:
                    acc = acc * alpha[:, None]
                ph, pl = split(p)
                t = ph @ vh[kc]
                if "drop_ph_vl" not in mut:
                    t = t + ph @ vl[kc]
                if "drop_pl_vh" not in mut:
                    t = t + pl @ vh[kc]
                acc = (acc.double() + t).float()
                m = mn
            parts.append((m, l, acc, False))
        if nsplit == 1 or (kps and ns == 1):
            o = parts[0][2] / parts[0][1][:, None]
        else:   # k_attn_combine
            M = torch.full((R,), -INF)
            for m, l, _, _ in parts:
                M = torch.maximum(M, m) if "merge_max_of_empty" in mut else torch.where(l > 0, torch.maximum(M, m), M)
            ls, o = torch.zeros(R), torch.zeros(R, hd)
            for m, l, acc, empty in parts:
                w = exp32(m - M)
                on = l > 0
                ls = torch.where(on, ls + l * w, ls)
                add = o + acc * w[:, None]
                o = add if "merge_no_skip_nan" in mut else torch.where(on[:, None], add, o)
            o = o / ls[:, None]
        out[:, kh * G:(kh + 1) * G] = o.view(tn, G, hd)
    return out.view(tn, H * hd)


_built = {}


def built(case):
    if case.name not in _built:
        _built[case.name] = (case.build(), {})
    return _built[case.name]


def refs(case, nsplit):
    data, cache = built(case)
    if nsplit not in cache:
        cache[nsplit] = ar.reference(case, data, nsplit)
    return data, cache[nsplit]


def family_ratios(case, mut=()):
    """{family: worst err / E of the emulation over the case's sequences and split settings}"""
    worst = {}
    hd, H = case.hd, case.H
    for nsplit, kps in case.splits:
        data, ref = refs(case, nsplit)
        for sq, (y, E, _) in zip(data, ref):
            got = emulate(sq.q, sq.K, sq.V, sq.nvis, H, case.KVH, case.kt, nsplit, kps, mut)
            for i in range(len(sq.nvis)):
                for h in range(H):
                    sl = slice(h * hd, (h + 1) * hd)
                    r = ar.ratio(got[i, sl], y[i, sl], E[i, sl])
                    worst[sq.fam[i][h]] = max(worst.get(sq.fam[i][h], 0.0), r)
    return worst


def hd_cases(hd, variants):
    return [c for c in ar.MFMA_CASES if c.hd == hd and c.variant in variants]


@pytest.mark.parametrize("case", ar.ALL_CASES, ids=lambda c: c.name)
def test_inputs_are_exact_and_within_the_ceiling(case):
    """Every case of the tables: the exactness properties (exact families), every family of the variant present, and
    E <= CEIL sum w |V| on every element for every split setting of the case."""
    data, _ = built(case)
    seen = {f for sq in data for row in sq.fam for f in row}
    want = {"A": ar.EXACT_A, "lo": ar.EXACT_LO, "wide": ("wide",), "o": ar.O_FAMILIES}[case.variant]
    assert seen == set(want), (case.name, set(want) - seen)
    if not case.exact:
        return
    for sq in data:
        ar.check_exact(sq, case.H, case.KVH)
        if case.bf16:
            assert torch.equal(sq.K.bfloat16().float(), sq.K) and torch.equal(sq.V.bfloat16().float(), sq.V)
    worst = 0.0
    for nsplit, _ in case.splits:
        for (y, E, S) in refs(case, nsplit)[1]:
            assert bool(torch.isfinite(y).all()) and bool((E > 0).all())
            assert bool((E <= ar.CEIL * S + 1e-30).all()), (case.name, float((E / (S + 1e-300)).max()))
            worst = max(worst, float((E / (S + 1e-300)).max()))
    print(f"{case.name}: max E / sum w|V| {worst:.2e}")


@pytest.mark.parametrize("case", [c for c in ar.MFMA_CASES + ar.GROUP_CASES if c.variant == "A"],
                         ids=lambda c: c.name)
def test_items_straddle_tile_and_split_edges(case):
    """A multi-row case has two tokens of one sequence either side of a tile edge and, for every setting with more than
    one split, either side of a split's first key; the rows of the later token include an `own` row."""
    data, _ = built(case)

    def straddles(edge_of):
        for sq, (L, tn) in zip(data, case.seqs):
            for i in range(tn - 1):
                if i // case.tpi != (i + 1) // case.tpi:
                    continue                                    # (the two tokens are in different items)
                last = min(tn, (i // case.tpi + 1) * case.tpi) - 1
                e = edge_of(sq.nvis[last])                      # the item's key count
                if e and any(sq.nvis[i] <= c < sq.nvis[i + 1] for c in e):
                    return True
        return False
    assert straddles(lambda L: range(case.kt, L, case.kt))
    for nsplit, kps in case.splits:
        if nsplit > 1:
            def edges(L):
                ns = ar.split_count(L, nsplit, kps)
                return range(ar.split_len(L, ns, case.kt), L, ar.split_len(L, ns, case.kt)) if ns > 1 else ()
            assert straddles(edges), (case.name, nsplit, kps)
    assert any(f == "own" for sq in data for row in sq.fam[1:] for f in row)


def test_bf16_split_residue():
    """hi + lo leaves at most RES |x| and |lo| <= LOB |x| (attn_ref's two format constants), on 2^20 random floats and
    on the worst case next to a power of two"""
    x = torch.cat([torch.randn(1 << 20, generator=ar.gen("split")) * 3,
                   torch.tensor([1 + 2.0 ** -8 + 2.0 ** -9 + 2.0 ** -17, 1 + 2.0 ** -8 - 2.0 ** -23])])
    hi, lo, res = ar.bf16_split(x)
    assert bool((res.abs() <= ar.RES * x.double().abs()).all()) and bool((lo.abs() <= ar.LOB * x.double().abs()).all())
    assert float((res.abs() / x.double().abs()).max()) > 2.0 ** -18      # (and no tighter power of two holds)
    p = torch.tensor([math.exp(-ar.LO_P_C)]).float()
    _, lo, _ = ar.bf16_split(p)
    assert abs(float(lo)) >= 2.0 ** -11 * float(p)                       # lo_p's common weight has a low half


@pytest.mark.parametrize("hd", [32, 64, 128])
def test_unmutated_emulation_is_within_the_bound(hd):
    for case in hd_cases(hd, ar.VARIANTS):
        worst = family_ratios(case)
        print(f"{case.name}: " + ", ".join(f"{f} {r:.3f}" for f, r in sorted(worst.items())))
        assert max(worst.values()) <= 1.0, (case.name, worst)


@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutant_exceeds_the_bound(hd, mut):
    fam = MUTANTS[mut]
    worst = 0.0
    for case in hd_cases(hd, ("lo",) if fam in ar.EXACT_LO else ("A",)):
        if case.kt == 32 and mut != "row_swap":
            continue                    # (the 2-wave case repeats the 8-wave one's families: once is enough here)
        worst = max(worst, family_ratios(case, (mut,)).get(fam, 0.0))
        if worst > 1.0:
            break
    print(f"hd {hd} {mut} on {fam}: err / E {worst:.3g}")
    assert worst > 1.0


def test_o_projection_bound_rejects_a_wrong_projection():
    """fo_attention_o's bound: a float32 restatement (the attention row rounded to float32, hi + lo against bf16 Wo, head
    partials in turn) stays within it; without the low half of the attention row, or with one head's slice of Wo
    shifted, it does not."""
    case = ar.O_CASE
    data, ref = refs(case, 1)
    oi = ar.o_inputs(case)
    att = torch.cat([y for y, _, _ in ref])
    Eatt = torch.cat([E for _, E, _ in ref])
    want = ar.o_proj(oi.x0, att, Eatt, oi.wo, oi.gamma, case.H, case.hd)

    def run(mut):
        a32 = att.float()
        hi, lo = split(a32)
        a = hi if mut == "no_lo" else hi + lo
        W = oi.wo.double()
        if mut == "head_shift":
            W = W.clone()
            W[:, :case.hd] = torch.roll(W[:, :case.hd], 1, dims=1)
        part = torch.stack([(a[:, h * case.hd:(h + 1) * case.hd] @ W[:, h * case.hd:(h + 1) * case.hd].t()).float()
                            for h in range(case.H)])
        v = torch.zeros_like(part[0])
        for h in range(case.H):
            v = v + part[h]
        x = oi.x0 + v
        return max(ar.ratio(x, want.x, want.Ex), ar.ratio(x * oi.gamma, want.yg, want.Eyg),
                   ar.ratio((x * x).sum(-1), want.ss, want.Ess))
    assert run(None) <= 1.0
    assert run("no_lo") > 1.0 and run("head_shift") > 1.0
