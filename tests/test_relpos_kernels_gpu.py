"""The speech encoder's rel-pos attention kernels (csrc/fo_attn.hip: k_relpos_fused, k_relpos_chunks +
k_relpos_chunks_append, k_enc_kv_write + k_relpos_attn), each launched through fo.ops between guards, against the
float64 session model of tests/relpos_ref.py: outputs within the derived bound, ring appends bit-equal, and every
byte a launch may not write bit-identical afterwards.  The sequence cases take all their metadata from
SpeechEncoderEngine.host_meta / advance.  tests/test_relpos_ref_cpu.py shows that the bound cannot hide a wrong
kernel.

Observed max(err / bound) on an MI355X: relpos_attention_fused 0.048 (head size 8; 0.0070 at head size 64, the case at
the table's last positions included), enc_kv_write + relpos_attention 0.044 (0.0079 at head size 64),
relpos_attention_chunks 0.048 (0.0075 at head size 64).  The bound is a worst case over every summation order; a
plain float32 restatement on the CPU sits at the same few thousandths of it.
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import relpos_ref as rr
from test_xpack_gpu import _check_packed_rb

pytestmark = pytest.mark.gpu
I32 = torch.int32


@pytest.fixture(scope="module")
def ops(dev):
    from fo import ops
    yield ops
    print("\nobserved max(err / bound):", {k: round(v, 4) for k, v in rr.OBSERVED.items() if k.startswith("relpos_")})


def _put(dev, t, ld=None, dtype=torch.float32):
    """t [..][D] inside a Guard (row stride ld for a matrix: the stride padding holds the sentinel)"""
    shape = list(t.shape)
    D = shape[-1]
    if ld:
        shape[-1] = ld
    g = rr.Guard(dev, *shape, dtype=dtype)
    g.t[..., :D] = t.to(dev)
    return g


def _launch(ops, dev, kind, h, dk, cap, B, T, qkv, ldq, ldo, kr, vr, meta, ring, ptab, bu, bv, scale, C=1, pack=False):
    """One launch of `kind` ("fused", "pair", "chunks") with every buffer guarded.  qkv [C B T][3 d] (chunk-major), kr /
    vr Guards that live across launches (their masks are set here), meta int [C][4 B] (start | len | ring | pstart;
    ring None: no ring array is passed).  -> (out [C B T][d] on the CPU, the packed halves' Guards or None)"""
    d = h * dk
    n = C * B * T
    qb = _put(dev, qkv, ldq)
    pb, bb = _put(dev, ptab), _put(dev, torch.stack([bu, bv]))
    mb = _put(dev, torch.as_tensor(np.asarray(meta, np.int32)).reshape(C, 4 * B), dtype=I32)
    ob = rr.Guard(dev, n, ldo)
    ob.mask[:, :d] = True
    kr.mask[:] = False
    for c in range(C):
        st, ln, rg = (np.asarray(meta).reshape(C, 4, B)[c, i] for i in range(3))
        for b in range(B):
            for t in range(T):
                kr.mask[int(rg[b]) if ring else b, (int(st[b]) + int(ln[b]) + t) % cap] = True
    vr.mask = kr.mask
    xp = None
    if pack:
        rb = (n + 15) // 16
        xp = NS(hi=rr.Guard(dev, d * 16 * rb, dtype=torch.bfloat16),
                lo=rr.Guard(dev, d * 16 * rb, dtype=torch.bfloat16))
        at = torch.arange(d * 16 * rb).view(d // 32, rb, 4, 16, 8).permute(1, 3, 0, 2, 4).reshape(rb * 16, d)[:n]
        for g in (xp.hi, xp.lo):     # the elements of rows < n in [d / 32][rb][4][16][8]
            g.mask[at.reshape(-1)] = True
    guards = [qb, pb, bb, mb, ob, kr, vr] + ([xp.hi, xp.lo] if pack else [])
    for g in guards:
        g.arm()
    m = mb.t
    q3 = qb.t[:, :3 * d]
    out = ob.t[:, :d]
    if kind == "chunks":
        assert ring
        ops.relpos_attention_chunks(q3, kr.t, vr.t, cap, m, B, C, pb.t, bb.t[0], bb.t[1], T, h, dk, scale, out)
    else:
        assert C == 1
        st, ln, rg, ps = m[0, :B], m[0, B:2 * B], (m[0, 2 * B:3 * B] if ring else None), m[0, 3 * B:]
        if kind == "fused":
            op = NS(hi=xp.hi.t, lo=xp.lo.t, K=d, rb=(n + 15) // 16) if pack else None
            ops.relpos_attention_fused(q3, kr.t, vr.t, cap, st, ln, rg, pb.t, ps, bb.t[0], bb.t[1], B, T, h, dk, scale,
                                       out, opack=op)
        else:
            ops.enc_kv_write(qb.t[:, d:2 * d], qb.t[:, 2 * d:3 * d], B, T, d, st, ln, rg, cap, kr.t, vr.t)
            ops.relpos_attention(qb.t[:, :d], kr.t, vr.t, cap, st, ln, rg, pb.t, ps, bb.t[0], bb.t[1], B, T, h, dk,
                                 scale, out)
    torch.cuda.synchronize(dev)
    got = ob.check(f"{kind} out")[:, :d]
    for g, what in ((qb, "q|k|v"), (pb, "position table"), (bb, "biases"), (mb, "metadata"), (kr, "K ring"),
                    (vr, "V ring")):
        g.check(f"{kind} {what}")
    if pack:
        xp.hi.check("packed hi")
        xp.lo.check("packed lo")
    return got, xp


def _rings(dev, data):
    kr, vr = rr.Guard(dev, *data.kr.shape), rr.Guard(dev, *data.vr.shape)
    kr.t.copy_(data.kr)
    vr.t.copy_(data.vr)
    return kr, vr


def _single(ops, dev, case, kind, B=None, pack=False):
    """the first B sessions of a single-launch case through `kind`: output within E, appended rows bit-equal"""
    data, y, E, _ = rr.single_ref(case)
    B = B or case.B
    T, d, cap = case.T, case.d, case.cap
    ring = data.ring is not None
    meta = case.start[:B] + case.lens[:B] + (data.ring[:B] if ring else [0] * B) + case.pstart[:B]
    kr, vr = _rings(dev, data)
    got, xp = _launch(ops, dev, kind, case.h, case.dk, cap, B, T, data.qkv[:B * T], case.ldq, case.ldo, kr, vr, meta,
                      ring, data.ptab, data.bu, data.bv, case.scale, pack=pack)
    r = rr.note("relpos_" + kind, rr.ratio(got, y[:B * T], E[:B * T]))
    print(f"{case.name} {kind}: max err/bound {r:.4f}")
    assert r <= 1.0
    krc, vrc = kr.t.cpu(), vr.t.cpu()
    for b in range(B):
        slot = data.ring[b] if ring else b
        at = [(case.start[b] + case.lens[b] + t) % cap for t in range(T)]
        assert torch.equal(krc[slot][at], data.qkv[b * T:(b + 1) * T, d:2 * d]), (case.name, b)
        assert torch.equal(vrc[slot][at], data.qkv[b * T:(b + 1) * T, 2 * d:]), (case.name, b)
    return got, xp, data, y


@pytest.mark.parametrize("case", rr.SINGLE_CASES, ids=lambda c: c.name)
def test_relpos_fused_matches_float64(ops, dev, case):
    got, _, data, y = _single(ops, dev, case, "fused")
    T, d = case.T, case.d
    if case.name == "one":
        for b, n in enumerate(case.lens):
            if n == 0:       # one key, weight 1.0: its own V row exactly
                assert torch.equal(got[b * T:(b + 1) * T], data.qkv[b * T:(b + 1) * T, 2 * d:])


@pytest.mark.parametrize("name,B", [("real7", 8), ("real7", 2), ("full8", 2)])
def test_relpos_fused_packed_output(ops, dev, name, B):
    """opack armed (56 rows; 14 rows, a partial row block; 16 rows, one full block): the XPack halves are the bf16 hi /
    lo split of the fp32 output the same launch wrote, bit for bit, and no packed row past the last is written."""
    case = next(c for c in rr.SINGLE_CASES if c.name == name)
    ops.launch_counts_reset()
    got, xp, _, _ = _single(ops, dev, case, "fused", B=B, pack=True)
    assert ops.launch_counts()["attn_opack"] == 1
    _check_packed_rb(NS(hi=xp.hi.t, lo=xp.lo.t), got.to(dev), B * case.T)


@pytest.mark.parametrize("case", [c for c in rr.SINGLE_CASES if c.T <= 8 and c.cap + c.T <= 264], ids=lambda c: c.name)
def test_enc_kv_write_then_relpos_attention_matches_float64(ops, dev, case):
    _single(ops, dev, case, "pair")


def _sequence(ops, dev, case, C):
    """The sequence in groups of at most C steps (C None: one fused launch per step), metadata from host_meta / advance
    on the stub: every chunk's output within E, and after each group the ring's live rows are the model's held rows."""
    from fo.speech import SpeechEncoderEngine as Eng
    data, ref, held = rr.seq_ref(case)
    stub = case.stub()
    kr, vr = _rings(dev, data)
    caches = rr.new_caches(case, data, kr.t, vr.t)
    pes = list(case.pe)
    T, d, cap = case.T, case.d, case.cap
    kind = "fused" if C is None else "chunks"
    sizes = []
    for s0, n in rr.groups(case, C or 1):
        act = rr.active(case, s0)
        cs = [caches[i] for i in act]
        B = len(act)
        metas = []
        for j in range(n):
            meta, new_pe = Eng.host_meta(stub, cs, [pes[i] for i in act])
            Eng.advance(stub, cs, T)
            for i, p in zip(act, new_pe):
                pes[i] = p
            metas.append(meta)
        qkv = torch.cat([data.qkv[s0 + j, i] for j in range(n) for i in act])
        got, _ = _launch(ops, dev, kind, case.h, case.dk, cap, B, T, qkv, 3 * d + 32, d + 16, kr, vr,
                         np.stack(metas), True, data.ptab, data.bu, data.bv, case.scale, C=n)
        for j in range(n):
            for k, i in enumerate(act):
                y, E = ref[s0 + j][i]
                r = rr.note("relpos_" + kind, rr.ratio(got[(j * B + k) * T:(j * B + k + 1) * T], y, E))
                assert r <= 1.0, (case.name, C, s0 + j, i, r)
        krc, vrc = kr.t.cpu(), vr.t.cpu()
        for i, c in zip(act, cs):
            K, V = held[s0 + n - 1][i]
            assert torch.equal(rr.live_rows(krc, c.slot, c.start, c.len, cap).double(), K), (case.name, C, s0, i)
            assert torch.equal(rr.live_rows(vrc, c.slot, c.start, c.len, cap).double(), V), (case.name, C, s0, i)
        sizes.append(n)
    return sizes


@pytest.mark.parametrize("name,C", [("seq_real", 1), ("seq_real", 3), ("seq_real", 8), ("seq_b", 1), ("seq_b", 3),
                                    ("seq_b", 8), ("seq_tiny", 4)])
def test_relpos_chunks_matches_float64(ops, dev, name, C):
    case = next(c for c in rr.SEQ_CASES if c.name == name)
    assert C * case.T <= case.cap
    sizes = _sequence(ops, dev, case, C)
    print(f"{name} C={C}: groups {sizes}, max err/bound so far {rr.OBSERVED['relpos_chunks']:.4f}")
    assert max(sizes) == C and (C == 1 or min(sizes) < C)        # a full group and a partial one


@pytest.mark.parametrize("case", rr.SEQ_CASES, ids=lambda c: c.name)
def test_relpos_fused_per_chunk_matches_float64(ops, dev, case):
    _sequence(ops, dev, case, None)
    print(f"{case.name} per-chunk fused: max err/bound so far {rr.OBSERVED['relpos_fused']:.4f}")


def test_full_ring_at_the_last_positions(ops, dev):
    """Real ring geometry (chunk 4, left 16), T = 7 on a full ring with pe % max_len at max_len - 2 and max_len - 1:
    the launch reads rows max_len and max_len + 1 of the position table.  The table is built as the engine builds
    it -- relpos_sinusoid at speech.pos_table_rows rows through the linear_pos PackedLinear -- and must itself
    reproduce float64 linear_pos(oracle.nets.rel_pe_table) at the same positions, per element within
        (2^-17 + gam(4 d)) sum |x| |w|   the bf16 hi + lo split of x keeps 2^-18 relative (2^-17 allowed); the 2 d
                                         products are exact in fp32 and their accumulation is allowed 2 U a term (the
                                         matrix unit's internal additions are not documented as round-to-nearest)
        + sum dx |w|                     dx = 2^-22 (1 + p div_k): torch's and numpy's float32 sin / cos may differ by
                                         an ulp each, and their float32 exp (div_k) by an ulp, which moves the
                                         argument p div_k by 2^-23 of itself (2^-22 allowed)."""
    from fo import speech, tables
    from fo.speech import SpeechEncoderEngine as Eng
    from oracle import nets
    h, dk, chunk, left, T = 4, 64, 4, 16, 7
    d = h * dk
    bs, fc, max_len, cap = speech.ring_geometry(chunk, left)
    rows = speech.pos_table_rows(max_len, fc, bs)
    g = rr.gen("relpos/lastrows")
    w = (rr.randn(g, d, d) / d ** 0.5).to(torch.bfloat16)
    tab = ops.PackedLinear(w.to(dev))(tables.relpos_sinusoid(rows, d).to(dev))
    torch.cuda.synchronize(dev)
    ptab = tab.cpu()
    assert ptab.shape == (rows, d)
    tail = np.arange(max_len - 80, rows)
    x64 = torch.from_numpy(nets.rel_pe_table(tail, d)).double()
    w64 = w.double()
    want = x64 @ w64.t()
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float64) * -(math.log(10000.0) / d))
    dx = 2.0 ** -22 * (1 + torch.from_numpy(tail).double()[:, None] * div).repeat_interleave(2, dim=1)
    bound = (2.0 ** -17 + rr.gam(4 * d)) * (x64.abs() @ w64.abs().t()) + dx @ w64.abs().t()
    assert rr.ratio(ptab[tail[0]:], want, bound) <= 1.0
    stub = NS(chunk=chunk, left=left, buffersize=bs, full_chunk=fc, max_len=max_len, cap=cap)
    B, slots = 2, 3
    caches = [NS(start=70, len=bs, slot=2), NS(start=9, len=bs, slot=0)]
    pes = [max_len - 2, 3 * max_len + max_len - 1]
    meta, _ = Eng.host_meta(stub, caches, pes)
    assert max(int(meta[3 * B + b]) + bs + T - 1 for b in range(B)) == max_len + 1 < rows
    data = NS(kr=rr.randn(g, slots, cap, d), vr=rr.randn(g, slots, cap, d))
    qkv = rr.randn(g, B * T, 3 * d)
    bu, bv = 0.3 * rr.randn(g, d), 0.3 * rr.randn(g, d)
    m = rr.Model(ptab, bu, bv, h, dk, chunk, bs, fc, max_len)
    kr, vr = _rings(dev, data)
    got, _ = _launch(ops, dev, "fused", h, dk, cap, B, T, qkv, 3 * d, d, kr, vr, meta, True, ptab, bu, bv,
                     rr.scale_of(dk), pack=False)
    for b, c in enumerate(caches):
        s = rr.Session(pes[b], rr.live_rows(data.kr, c.slot, c.start, c.len, cap),
                       rr.live_rows(data.vr, c.slot, c.start, c.len, cap), d)
        r_ = qkv[b * T:(b + 1) * T]
        y, E = m.step(s, r_[:, :d], r_[:, d:2 * d], r_[:, 2 * d:])
        r = rr.note("relpos_fused", rr.ratio(got[b * T:(b + 1) * T], y, E))
        print(f"last rows, session {b}: max err/bound {r:.4f}")
        assert r <= 1.0
