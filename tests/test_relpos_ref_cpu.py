"""tests/relpos_ref.py on the CPU: each listed mutant of the rel-pos attention leaves the derived bound on at least one
table case (and the model's ring state where it touches the ring), the bound stays under the tolerance the fused
encoder block is already granted, the exact rows come out of the model as stated, SpeechEncoderEngine.host_meta /
advance keep a CPU ring equal to the model's held rows through every sequence case, and the position table the
engine allocates covers every row its own metadata can make a kernel read.

`peaked` is exempt from the ceiling: session 0's queries are 8 times larger, and the bound on a score (and with it on
a weight) grows with |q|; its greatest bound is 7.4e-4 of max|y| (printed below).  Every mutant that a single launch
can show still leaves it there, so the bound is not vacuous."""
import pytest
import torch

import relpos_ref as rr
from fo import speech
from fo.speech import SpeechEncoderEngine as Eng


def _over(got, y, E):
    got = got.float()
    return (not bool(torch.isfinite(got).all())) or rr.ratio(got, y, E) > 1.0


def _same_rows(live, held):
    return all(a.shape == b.shape and torch.equal(a.double(), b) for a, b in zip(live, held))


def _single_verdict(case, mut):
    """(output leaves the bound, ring state differs from the model's) for a mutant on a single-launch case"""
    data, y, E, held = rr.single_ref(case)
    if mut in rr.MUT_MODEL:
        return _over(rr.single_ref(case, (mut,))[1], y, E), False
    if mut.startswith("trim"):
        return False, False          # (advance's rule: the sequence cases)
    out, kr, vr = rr.single_cpu(case, (mut,))
    ring_off = False
    for b in range(case.B):
        st, n = rr.after_advance(case, b)
        slot = data.ring[b] if data.ring else b
        live = (rr.live_rows(kr, slot, st, n, case.cap), rr.live_rows(vr, slot, st, n, case.cap))
        ring_off |= not _same_rows(live, held[b])
    return _over(out, y, E), ring_off


def _seq_verdict(case, mut):
    _, ref, held = rr.seq_ref(case)
    if mut in rr.MUT_MODEL:
        # the mutated attention on the right bookkeeping
        out, live = rr.seq_cpu(case, Eng, (mut,))
    else:
        out, live = rr.seq_cpu(case, Eng, mut)
    over = any(_over(out[s][i], *ref[s][i]) for s in range(case.steps) for i in out[s])
    ring_off = any(not _same_rows(live[s][i], held[s][i]) for s in range(case.steps) for i in live[s])
    return over, ring_off


@pytest.mark.parametrize("mut", rr.MUTANTS)
def test_mutant_leaves_the_bound(mut):
    hits, ring_hits = [], []
    for case in rr.SINGLE_CASES:
        o, r = _single_verdict(case, mut)
        hits += [case.name] * o
        ring_hits += [case.name] * r
    for case in rr.SEQ_CASES:
        o, r = _seq_verdict(case, mut)
        hits += [case.name] * o
        ring_hits += [case.name] * r
    print(f"{mut}: leaves the bound on {hits}; ring state differs on {ring_hits}")
    assert hits
    # peaked's bound is not vacuous (late / trim show in a later chunk only: the sequence cases)
    assert "peaked" in hits or mut in ("late", "trim-1", "trim+1")
    if mut in rr.MUT_RING:
        assert ring_hits


@pytest.mark.parametrize("case", rr.SINGLE_CASES + rr.SEQ_CASES, ids=lambda c: c.name)
def test_bound_ceiling(case):
    if case in rr.SINGLE_CASES:
        _, y, E, _ = rr.single_ref(case)
        pairs = [(y, E)]
    else:
        pairs = [v for o in rr.seq_ref(case)[1] for v in o.values()]
    worst = max(float(E.max()) / float(y.abs().max()) for y, E in pairs)
    print(f"{case.name}: greatest bound {worst:.3e} of max|y|")
    assert all(bool((E > 0).all()) for _, E in pairs)
    if case.name != "peaked":
        assert worst <= rr.CEIL


@pytest.mark.parametrize("case", rr.SINGLE_CASES, ids=lambda c: c.name)
def test_float32_restatement_stays_inside_the_bound(case):
    """the operation in plain float32 torch (another summation order than any kernel's): the bound is within a
    correct kernel's reach"""
    data, y, E, _ = rr.single_ref(case)
    d, T, dk = case.d, case.T, case.dk
    out = torch.empty(case.B * T, d)
    sc = torch.tensor(case.scale, dtype=torch.float32)
    for b in range(case.B):
        r = data.qkv[b * T:(b + 1) * T]
        K, V = torch.cat([data.K0[b], r[:, d:2 * d]]), torch.cat([data.V0[b], r[:, 2 * d:]])
        P = data.ptab[case.pstart[b]:case.pstart[b] + K.shape[0]]
        for hh in range(case.h):
            sl = slice(hh * dk, (hh + 1) * dk)
            s = ((r[:, sl] + data.bu[sl]) @ K[:, sl].t() + (r[:, sl] + data.bv[sl]) @ P[:, sl].t()) * sc
            e = torch.exp(s - s.max(-1, keepdim=True).values)
            out[b * T:(b + 1) * T, sl] = (e * (1.0 / e.sum(-1, keepdim=True))) @ V[:, sl]
    worst = rr.ratio(out, y, E)
    print(f"{case.name}: float32 restatement max err/bound {worst:.4f}")
    assert worst <= 1.0


def test_exact_rows():
    case = next(c for c in rr.SINGLE_CASES if c.name == "one")
    data, y, E, _ = rr.single_ref(case)
    d = case.d
    for b, n in enumerate(case.lens):
        if n == 0:      # one key of weight 1.0: the row is its own V row, exactly
            assert torch.equal(y[b * case.T:(b + 1) * case.T], data.qkv[b * case.T:(b + 1) * case.T, 2 * d:].double())
    case = next(c for c in rr.SINGLE_CASES if c.name == "peaked")
    data, y, E, held = rr.single_ref(case)
    T = case.T
    V = torch.cat([data.V0[1].double(), data.qkv[T:2 * T, 2 * d:].double()])
    assert rr.ratio(V.mean(0).expand(T, d), y[T:2 * T], E[T:2 * T]) <= 1.0      # uniform weights: the mean of V


@pytest.mark.parametrize("case", rr.SEQ_CASES, ids=lambda c: c.name)
def test_bookkeeping_on_a_cpu_ring(case):
    """host_meta / advance (the product's, unbound on a stub) against the model: after every step the rows (start +
    j) % cap, j < len, of the session's slot are the model's held rows in order, and the outputs computed through
    that metadata are the model's."""
    _, ref, held = rr.seq_ref(case)
    out, live = rr.seq_cpu(case, Eng)
    seen_empty_beside_full = wrapped_full = False
    for s in range(case.steps):
        assert set(live[s]) == set(rr.active(case, s))
        for i in live[s]:
            assert _same_rows(live[s][i], held[s][i]), (s, i)
            assert not _over(out[s][i], *ref[s][i]), (s, i)
    # the conditions the case table promises, from the model alone
    m = case.max_len
    for i in range(4):
        pe = case.pe[i]
        for s in range(case.join[i], case.steps):
            n_before = case.init[i][0] if s == case.join[i] else held[s - 1][i][0].shape[0]
            full = n_before == case.buffersize
            if full and pe >= m:
                wrapped_full = True
            prev = held[s - 1] if s else {}
            if n_before == 0 and any(kv[0].shape[0] == case.buffersize for kv in prev.values()):
                seen_empty_beside_full = True
            top = max(0, pe % m - case.full_chunk) + n_before + case.T - 1
            assert top < m, (i, s, top)          # every row read lies inside a max_len-row table
            pe = pe % m + case.chunk
    assert seen_empty_beside_full
    assert wrapped_full or case.name == "seq_b"          # (seq_b stays away from the wrap)


def test_position_table_covers_every_row_the_metadata_can_reach():
    """Real geometry: every pe_index in [0, max_len), every T the engine admits and a full ring -- the largest row
    the kernels read (pstart + len + T - 1, pstart from the engine's own host_meta) lies inside the table the engine
    allocates (speech.pos_table_rows, the row count __init__ uses)."""
    from types import SimpleNamespace as NS

    from oracle import configs
    tr = configs.get("real")["train_yaml"]["encoder_conf"]["para_conf"]["transformer"]
    chunk, left = tr["transformer-chunk_size"], tr["transformer-left_chunks"]
    bs, fc, max_len, cap = speech.ring_geometry(chunk, left)
    stub = NS(chunk=chunk, left=left, buffersize=bs, full_chunk=fc, max_len=max_len, cap=cap)
    rows = speech.pos_table_rows(max_len, fc, bs)
    c = NS(start=0, len=bs, slot=0)
    worst = {}
    for pe in range(max_len):
        meta, _ = Eng.host_meta(stub, [c], [pe])
        for T in range(1, speech.ENC_MAX_T + 1):
            worst[T] = max(worst.get(T, 0), int(meta[3]) + int(meta[1]) + T - 1)
    print(f"table rows {rows} (max_len {max_len}); largest row read per T: {worst}")
    assert all(top < rows for top in worst.values()), (rows, worst)
    assert rows - max_len <= speech.ENC_MAX_T          # a handful of rows, not a second table
    assert cap >= bs + speech.ENC_MAX_T
