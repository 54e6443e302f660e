"""The paged attention kernels (csrc/fo_attn.hip, csrc/fo_attn_rows.h) against tests/attn_ref.py's float64 model
within its derived bound, on inputs whose scores are exact in the kernels' arithmetic and on a poisoned pool.

Poison protocol, every case: pool K / V (codes and scales of an FP8 pool) start as NaN and only the slots of the keys
some row may see are written; a page no sequence owns stays NaN and fills every unused block-table entry; part_ml /
part_o start as NaN; out lies between helper_ref.Guard rows; tickets come back zero and ticketed launches run twice;
any NaN in out fails.  Sequences fork from a one-key base (its partial page is copied on write) in a pool whose free
list was stirred first, so their pages are neither contiguous nor ascending.  Every row and element is compared:
max(err / E) <= 1 per case.  A bf16 pool holding the same values (the variants whose K / V are bf16 values) must give
the fp32 pool's result bit for bit, and on e4m3-quantised rows the fp32, bf16 and e4m3 pools give one result, also
held to E.  tests/test_attn_ref_cpu.py shows that E rejects wrong kernels.

Observed max(err / E) on an MI355X (this file's run; the table it prints at its end is the source), per form and
variant -- A: the exact families whose K / V are bf16 values, lo: lo_k and lo_v, wide: the inexact family, e4m3: the
quantised rows:
    form                       A       lo      wide     e4m3
    k_attn_mfma<32>            0.214   0.390   0.0363   0.0296
    k_attn_mfma<64>            0.225   0.532   0.0214   0.0247
    k_attn_mfma<128, 8>        0.241   0.291   0.0219   0.0194
    k_attn_mfma<128, 8, 2>     0.193   0.263   0.0167   0.0038
    k_attn_mfma<128, 2>        0.222   0.285   0.0118   -
    chunk-major group          0.381   0.451   -        -
    k_attn_gqa_decode<128>     0.189   0.274   0.0221   0.0011
    k_attn_decode<32>          0.0897  0.0819  0.0222   -
    k_attn_decode<64>          0.0885  0.109   0.0153   -
    k_attn_decode<128>         0.0835  0.157   0.00928  -
    k_attn_decode_o<64>        0.00824 (x, yg and the sum of squares)
No NaN, every guard and ticket intact, every bf16 / e4m3 equality held.  (The CPU emulation of
tests/test_attn_ref_cpu.py, which adds a tile's exact bf16 products in float64, sits in the same 0.2 .. 0.5 on the
MFMA forms' A and lo variants.)
The wide family against plain float64 attention -- what the three-product scheme costs at scores of several hundred,
where the dropped low-by-low product and the residues of q and K move a score by up to 2^-15 of sum |q k|: max |err|
3.3e-3 .. 8.6e-3 (2e-3 .. 3e-3 of sum w |V|) on the MFMA forms, against 1.4e-4 .. 2.1e-4 (5e-5 .. 9e-5) on the
fp32 decode forms.
"""
import pytest
import torch

import attn_ref as ar

pytestmark = pytest.mark.gpu
PS = 16
NAN = float("nan")
KERNEL = {"mfma32": "k_attn_mfma<32>", "mfma64": "k_attn_mfma<64>", "mfma128x8": "k_attn_mfma<128, 8>",
          "mfma128x8x2": "k_attn_mfma<128, 8, 2>", "mfma128x2": "k_attn_mfma<128, 2>", "group128": "chunk-major group",
          "gqa128": "k_attn_gqa_decode<128>", "decode32": "k_attn_decode<32>", "decode64": "k_attn_decode<64>",
          "decode128": "k_attn_decode<128>", "decode_o64": "k_attn_decode_o<64>"}
COUNTER = {"mfma": "attn_mfma", "gqa": "attn_gqa_decode", "fp32": "attn_decode"}
FAMILIES = ("attn_mfma", "attn_decode", "attn_gqa_decode", "attn_o")


@pytest.fixture(scope="module")
def fo(dev):
    from fo import kv, ops, quant
    from types import SimpleNamespace
    yield SimpleNamespace(kv=kv, ops=ops, quant=quant)
    print("\nobserved max(err / E), and the wide family's error against plain float64 attention:")
    for k, v in sorted(ar.OBSERVED.items()):
        print(f"    {k:48s} {v:.3g}")


def poisoned_pool(fo, dev, KVH, hd, n_pages, dtype=torch.float32):
    pool = fo.kv.KVPool(1, KVH, hd, n_pages, PS, dev, dtype=dtype)
    if pool.fp8:
        pool.k.view(torch.uint8).fill_(0x7F)
        pool.v.view(torch.uint8).fill_(0x7F)
        pool.ks.fill_(NAN)
        pool.vs.fill_(NAN)
    else:
        pool.k.fill_(NAN)
        pool.v.fill_(NAN)
    return pool


class Setup:
    """The pools, sequences and launch tables of one case; rows[s]: the out rows of sequence s's tokens."""

    def __init__(self, fo, dev, case, data, group=None):
        self.fo, self.dev, self.case, self.data = fo, dev, case, data
        KVH, hd, G = case.KVH, case.hd, case.H // case.KVH
        n_pages = sum(-(-L // PS) + 1 for L, _ in case.seqs) + 30
        self.pool = pool = poisoned_pool(fo, dev, KVH, hd, n_pages)
        held = [pool.alloc() for _ in range(24)]          # stir the free list; two pages stay out as holes
        for i in (3, 17, 0, 22, 9, 5, 14, 1, 20, 11, 6, 23, 2, 16, 8, 19, 4, 12, 21, 10, 15, 18):
            pool.release(held[i])
        self.trap = held[7]                               # no sequence owns it: NaN to the end
        base = fo.kv.KVSeq(pool)
        fo.kv.BatchMeta([(base, 1, 0, True)], dev)
        self.seqs, forks = [], []
        for L, tn in case.seqs:
            old = L - tn
            s = base.fork() if old >= 1 else fo.kv.KVSeq(pool)
            if old >= 1:
                forks.append(s)
            if old > 1:
                fo.kv.BatchMeta([(s, old - 1, 1, True)], dev)
            self.seqs.append(s)
        if group is None:
            self.meta = meta = fo.kv.BatchMeta([(s, tn, s.length, True) for s, (_, tn) in zip(self.seqs, case.seqs)],
                                               dev, gqa=G, rows=case.rows)
            t0 = [sum(tn for _, tn in case.seqs[:i]) for i in range(len(case.seqs))]
            self.rows = [list(range(t, t + tn)) for t, (_, tn) in zip(t0, case.seqs)]
            bt_dev = meta.block_table
        else:
            gm = fo.kv.GroupMeta(group.B, group.To, group.C, G, 256, PS, dev)
            hbuf = torch.zeros(gm.size, dtype=torch.int32)
            gm.fill(hbuf.numpy(), self.seqs, group.C)
            gm.buf.copy_(hbuf)
            self.gm, self.meta = gm, gm.metas[group.C]
            n1 = group.B * group.To
            self.rows = [[j * n1 + b * group.To + i for j in range(group.C) for i in range(group.To)]
                         for b in range(group.B)]
            bt_dev = self.meta.block_table
        assert [s.length for s in self.seqs] == [L for L, _ in case.seqs]
        assert sum(s.pages[0] != base.pages[0] for s in forks) >= len(forks) - 1             # copy-on-write ran
        assert any(s.pages != sorted(s.pages) for s in self.seqs)                            # pages not ascending
        bt = torch.full(tuple(bt_dev.shape), self.trap, dtype=torch.int32)
        for i, s in enumerate(self.seqs):
            bt[i, :len(s.pages)] = torch.tensor(s.pages, dtype=torch.int32)
        bt_dev.copy_(bt)
        self.T = self.meta.T
        self.slots = [torch.tensor([s.slot(p) for p in range(L)], dtype=torch.long, device=dev)
                      for s, (L, _) in zip(self.seqs, case.seqs)]
        q = torch.zeros(self.T, case.H * hd)
        for sq, rows in zip(data, self.rows):
            q[rows] = sq.q.reshape(len(rows), -1)
        self.q = q.to(dev)
        self.fill(pool, [sq.K for sq in data], [sq.V for sq in data])
        self.ref = {}

    def fill(self, pool, Ks, Vs):
        """the sequences' keys into a pool: only the slots some row may see"""
        for sl, K, V in zip(self.slots, Ks, Vs):
            if pool.fp8:
                for name, x in (("k", K), ("v", V)):
                    codes, e, img = self.fo.quant.quantize_kv_rows(x)
                    assert torch.equal(img.float(), x), "an FP8 pool takes rows that are their own e4m3 image"
                    getattr(pool, name)[0].view(torch.uint8)[sl // PS, :, sl % PS] = codes.to(self.dev)
                    scl = torch.ldexp(torch.ones(e.shape), e)
                    getattr(pool, name + "s")[0][sl // PS, :, sl % PS] = scl.to(self.dev)
            else:
                pool.k[0][sl // PS, :, sl % PS] = K.to(self.dev, pool.dtype)
                pool.v[0][sl // PS, :, sl % PS] = V.to(self.dev, pool.dtype)

    def twin(self, dtype):
        c = self.case
        return poisoned_pool(self.fo, self.dev, c.KVH, c.hd, self.pool.n_pages, dtype)

    def reference(self, nsplit, data=None, exact=None):
        key = (nsplit, id(data))
        if key not in self.ref:
            c = self.case
            self.ref[key] = [ar.attend(sq.q, sq.K, sq.V, sq.nvis, c.H, c.KVH, ar.seq_form(c, L), c.kt, c.nw, nsplit,
                                       c.exact if exact is None else exact)
                             for sq, (L, _) in zip(data or self.data, c.seqs)]
        return self.ref[key]

    def launch(self, pool, nsplit, kps, what):
        """-> out [T][H hd] on the CPU; the protocol's checks around the launch"""
        ops, c, dev, T = self.fo.ops, self.case, self.dev, self.T
        meta = self.meta
        part_ml = torch.full((T * c.H * nsplit * 2,), NAN, device=dev) if nsplit > 1 else None
        part_o = torch.full((T * c.H * nsplit * c.hd,), NAN, device=dev) if nsplit > 1 else None
        tickets = torch.zeros(meta.n_items * c.KVH, dtype=torch.int32, device=dev) if kps else None
        scales = dict(kscale=pool.ks[0], vscale=pool.vs[0]) if pool.fp8 else {}
        outs = []
        for _ in range(2 if kps else 1):
            g = ar.Guard(dev, T, c.H * c.hd)
            g.t.fill_(NAN)
            g.mask[:] = True
            g.arm()
            ops.launch_counts_reset()
            ops.attention(self.q, T, meta.items, meta.n_items, meta.max_rows, meta.tok_nvis, meta.block_table, PS,
                          pool.k[0], pool.v[0], c.H, c.KVH, c.hd, ar.SCALE, nsplit, part_ml, part_o, g.t,
                          tickets=tickets, keys_per_split=kps or 128, **scales)
            torch.cuda.synchronize()
            cnt = ops.launch_counts()
            assert cnt[COUNTER[c.form]] == 1 and sum(cnt[k] for k in FAMILIES) == 1, (what, cnt)
            got = g.check(what)
            assert not bool(torch.isnan(got).any()), f"{what}: NaN in out (a slot that holds no key was read)"
            if kps:
                assert int(tickets.abs().sum()) == 0, what
            outs.append(got)
        if kps:
            assert torch.equal(outs[0], outs[1]), f"{what}: the second launch differs"
        kp = pool.k[0][self.trap]
        assert bool(torch.isnan(kp.float() if not pool.fp8 else pool.ks[0][self.trap]).all()), what
        return outs[0]

    def worst(self, got, ref):
        r = 0.0
        for rows, (y, E, _) in zip(self.rows, ref):
            r = max(r, ar.ratio(got[rows], y, E))
        return r


_setups = {}


def setup_of(fo, dev, case, group=None):
    if case.name not in _setups:
        _setups[case.name] = Setup(fo, dev, case, case.build(), group)
    return _setups[case.name]


def run_case(fo, dev, case, group=None):
    su = setup_of(fo, dev, case, group)
    base = case.name.split("/")[0]
    assert su.meta.max_rows == (1 if case.form == "fp32" else case.H // case.KVH if case.form == "gqa" else
                                max(min(tn, case.tpi) for _, tn in case.seqs) * (case.H // case.KVH))
    p16 = None
    if case.bf16 and case.form != "fp32":
        p16 = su.twin(torch.bfloat16)
        su.fill(p16, [sq.K for sq in su.data], [sq.V for sq in su.data])
    worst = 0.0
    for nsplit, kps in case.splits:
        what = f"{case.name} ns {nsplit} kps {kps}"
        got = su.launch(su.pool, nsplit, kps, what)
        r = su.worst(got, su.reference(nsplit))
        if case.variant == "wide":     # what the three-product scheme costs at scores of several hundred
            ref = su.reference(nsplit)
            ar.note(f"{KERNEL[base]} wide: max |err|", max(float((got[rows].double() - y).abs().max())
                                                           for rows, (y, _, _) in zip(su.rows, ref)))
            ar.note(f"{KERNEL[base]} wide: max |err| / sum w|V|", max(float(((got[rows].double() - y).abs() / S).max())
                                                                      for rows, (y, _, S) in zip(su.rows, ref)))
        print(f"{what}: max err/E {r:.4f}")
        worst = max(worst, r)
        assert r <= 1.0, what
        if p16 is not None and not (case.kt == 32):       # (the 2-wave form reads an fp32 cache only)
            got16 = su.launch(p16, nsplit, kps, what + " bf16")
            assert torch.equal(got16, got), f"{what}: the bf16 pool's result differs from the fp32 pool's"
    ar.note(f"{KERNEL[base]} {case.variant}", worst)


@pytest.mark.parametrize("case", ar.MFMA_CASES, ids=lambda c: c.name)
def test_multi_row_forms(fo, dev, case):
    """attn_rows_body in its five instantiations: one split, static splits + k_attn_combine, ticketed splits merged in
    the launch; the exact families on an fp32 and a bf16 pool, the lo_k / lo_v and wide variants on fp32."""
    if case.rows == 32:
        assert fo.ops.attn_max_rows(128) == 32
    run_case(fo, dev, case)


@pytest.mark.parametrize("case", ar.GROUP_CASES, ids=lambda c: c.name)
def test_chunk_major_group(fo, dev, case):
    """kv.GroupMeta's tables: 4 sessions x 4 chunks of 2 tokens, rows chunk-major, ragged odd key counts, one session's
    item across the 128-key tile and split edge."""
    run_case(fo, dev, case, ar.GROUP)


@pytest.mark.parametrize("case", ar.GQA_CASES, ids=lambda c: c.name)
def test_gqa_decode(fo, dev, case):
    """k_attn_gqa_decode<128>: the single-row fp32 body up to GQA_DEC_KEYS = 448 keys (csrc/fo_attn.hip; the measured
    crossover recorded there) and the multi-row MFMA body beyond, chosen per item in one launch -- the model takes the
    bound's form per item the same way (attn_ref.seq_form)."""
    run_case(fo, dev, case)


@pytest.mark.parametrize("case", ar.DECODE_CASES, ids=lambda c: c.name)
def test_single_row_decode(fo, dev, case):
    """k_attn_decode<32 / 64 / 128>: one token a sequence, one query head per kv head."""
    run_case(fo, dev, case)


E4M3_CASES = [c for c in ar.MFMA_CASES + ar.GQA_CASES if c.variant == "A" and c.kt != 32]


@pytest.mark.parametrize("case", E4M3_CASES, ids=lambda c: c.name)
def test_e4m3_rows_on_three_pools(fo, dev, case):
    """The case's K / V rows quantised on the CPU (fo.quant.quantize_kv_rows); the dequantised rows are the common
    values of an fp32, a bf16 and an e4m3 pool: one result bit for bit, and the fp32 pool's within E of the model on
    those values (the general bound: quantised rows are not the exact construction).  The 2-wave form and one row per
    item have no FP8 kernel and are left out."""
    su = setup_of(fo, dev, case)
    from types import SimpleNamespace as NS
    data8 = []
    for sq in su.data:
        K8, V8 = (fo.quant.quantize_kv_rows(x)[2].float() for x in (sq.K, sq.V))
        data8.append(NS(q=sq.q, K=K8, V=V8, nvis=sq.nvis, fam=sq.fam))
    Ks, Vs = [d.K for d in data8], [d.V for d in data8]
    pools = [su.twin(dt) for dt in (torch.float32, torch.bfloat16, torch.float8_e4m3fn)]
    for p in pools:
        su.fill(p, Ks, Vs)
    base = case.name.split("/")[0]
    worst = 0.0
    for nsplit, kps in case.splits:
        what = f"{case.name} e4m3 rows ns {nsplit} kps {kps}"
        o32, o16, o8 = (su.launch(p, nsplit, kps, what) for p in pools)
        assert torch.equal(o8, o16) and torch.equal(o8, o32), what
        r = su.worst(o32, su.reference(nsplit, data8, exact=False))
        print(f"{what}: max err/E {r:.4f}")
        worst = max(worst, r)
        assert r <= 1.0, what
    ar.note(f"{KERNEL[base]} e4m3 rows", worst)


def test_decode_fused_with_o_projection(fo, dev):
    """fo_attention_o: x + att Wo^T in place, yg = x gamma and the row's sum of squares, every element against its own
    bound (attn_ref.o_proj); part starts as NaN, x and yg lie between guards, the tickets come back zero."""
    ops, case = fo.ops, ar.O_CASE
    su = setup_of(fo, dev, case)
    oi = ar.o_inputs(case)
    B, H, hd, D = len(case.seqs), case.H, case.hd, oi.D
    ref = su.reference(1)
    att, Eatt = torch.cat([y for y, _, _ in ref]), torch.cat([E for _, E, _ in ref])
    want = ar.o_proj(oi.x0, att, Eatt, oi.wo, oi.gamma, H, hd)
    lin = ops.PackedLinear(oi.wo.to(dev))
    x, yg = ar.Guard(dev, B, D), ar.Guard(dev, B, D)
    x.t.copy_(oi.x0)
    yg.t.fill_(NAN)
    x.mask[:] = True
    yg.mask[:] = True
    x.arm()
    yg.arm()
    st = ops.RowStats(B, dev)
    st.buf.fill_(NAN)
    part = torch.full((B * H * D,), NAN, device=dev)
    tickets = torch.zeros(B, dtype=torch.int32, device=dev)
    ops.launch_counts_reset()
    ops.attention_o(su.q, B, None, su.meta.tok_nvis, su.meta.block_table, PS, su.pool.k[0], su.pool.v[0], H, hd,
                    ar.SCALE, lin, part, tickets, x.t, oi.gamma.to(dev), yg.t, st)
    torch.cuda.synchronize()
    cnt = ops.launch_counts()
    assert cnt["attn_o"] == 1 and sum(cnt[k] for k in FAMILIES) == 1 and st.groups == 1, cnt
    assert int(tickets.abs().sum()) == 0
    gx, gy, ss = x.check("x"), yg.check("yg"), st.buf[:B].cpu()
    assert not bool(torch.isnan(gx).any() or torch.isnan(gy).any() or torch.isnan(ss).any())
    r = max(ar.ratio(gx, want.x, want.Ex), ar.ratio(gy, want.yg, want.Eyg), ar.ratio(ss, want.ss, want.Ess))
    print(f"fo_attention_o: max err/E {ar.note(KERNEL['decode_o64'], r):.4f}")
    assert r <= 1.0
