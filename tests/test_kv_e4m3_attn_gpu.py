"""fo_attention_kv8 on an FP8 (e4m3) paged KV against fo_attention_kv on a bf16 pool and on an fp32 pool
that hold the same values.

The FP8 pool holds e4m3fn codes and one scale 2^e per (token, kv head); code * 2^e has at most 4 significant bits, so
it is exactly a bf16 value, and the FP8 kernels decode to those bf16 values before any arithmetic and are the bf16
kernels from there.  The three results must therefore be EQUAL (torch.equal on the floats), for every kernel form with
an FP8 instantiation: the 8-wave multi-row kernel with one split, the in-launch merge and the combine launch, its
two-row-tile form, the 4-wave kernels at head_dim 64 and 32, and the one-token GQA launch on both of its bodies.  All
are also held to the project's attention tolerance, 2e-5 abs, against a float64 softmax attention on those values.

Values: every K / V row is randn * 2^u with an integer u drawn per (token, kv head) from {-4..0}, quantised on the CPU
by fo.quant.quantize_kv_rows; the codes and scales go into the FP8 pool and the bf16 image into the other two.  The
rows' exponents differ (at least 5 distinct ones per case of 64 rows or more), so a scale read from the wrong key
changes the result.  Magnitudes do not exceed tests/test_kv_bf16_attn_gpu.py's, whose tolerance carries over.  Pages
are dealt in a shuffled order; the fp32 and bf16 pools are pre-filled with NaN, the codes with the NaN byte 0x7f and
the scales with NaN, so a read outside a session's keys shows.
"""
import random

import pytest
import torch

from fo import ops
from fo.kv import KVPool, KVSeq
from fo.quant import quantize_kv_rows

pytestmark = pytest.mark.gpu
PS = 16
ATOL = 2e-5   # the project's attention tolerance (tests/test_attn_gpu.py's MFMA bound)
FAMILIES = ("attn_mfma", "attn_decode", "attn_gqa_decode")


class Case:
    """sessions: [(keys, tokens)]: each session holds `keys` keys and the launch carries its last `tokens` tokens,
    causal (token i of tn sees keys - (tn - 1 - i), at least 1).  One work item per session.  Builds the three pools,
    the launch tables, q and the float64 reference once."""

    def __init__(self, dev, H, KVH, hd, sessions, seed):
        g = torch.Generator().manual_seed(seed)
        n_pages = sum((L + PS - 1) // PS for L, _ in sessions) + 5
        self.dev, self.H, self.KVH, self.hd, self.sessions = dev, H, KVH, hd, sessions
        self.p32 = KVPool(1, KVH, hd, n_pages, PS, dev)
        self.p16 = KVPool(1, KVH, hd, n_pages, PS, dev, dtype=torch.bfloat16)
        self.p8 = KVPool(1, KVH, hd, n_pages, PS, dev, dtype=torch.float8_e4m3fn)
        assert self.p8.k.dtype == torch.float8_e4m3fn and self.p8.k.shape == self.p32.k.shape
        random.Random(seed).shuffle(self.p32.free)   # pages dealt in a shuffled, non-contiguous order
        for p in (self.p32, self.p16):
            p.k.fill_(float("nan"))
            p.v.fill_(float("nan"))
        for t in (self.p8.k, self.p8.v):
            t.view(torch.uint8).fill_(0x7F)
        for t in (self.p8.ks, self.p8.vs):
            t.fill_(float("nan"))
        self.seqs, items, nvis, t = [], [], [], 0
        exps, n_rows = set(), 0
        for s, (L, tn) in enumerate(sessions):
            seq = KVSeq(self.p32)
            seq.reserve(L)
            seq.length = L
            self.seqs.append(seq)
            sl = torch.tensor([seq.slot(p) for p in range(L)], dtype=torch.long, device=dev)
            for name in ("k", "v"):
                u = torch.randint(-4, 1, (L, KVH, 1), generator=g)
                x = torch.ldexp(torch.randn(L, KVH, hd, generator=g), u)
                q, e, img = quantize_kv_rows(x)
                exps |= set(e.flatten().tolist())
                n_rows += e.numel()
                getattr(self.p8, name)[0].view(torch.uint8)[sl // PS, :, sl % PS] = q.to(dev)
                getattr(self.p8, name + "s")[0][sl // PS, :, sl % PS] = torch.ldexp(torch.ones(L, KVH), e).to(dev)
                getattr(self.p16, name)[0][sl // PS, :, sl % PS] = img.to(dev)
                getattr(self.p32, name)[0][sl // PS, :, sl % PS] = img.float().to(dev)
            items += [s, t, tn]
            nvis += [max(1, L - (tn - 1 - i)) for i in range(tn)]
            t += tn
        assert n_rows < 64 or len(exps) >= 5, (n_rows, exps)
        self.T, self.n_items = t, len(sessions)
        self.max_rows = max(tn for _, tn in sessions) * (H // KVH)
        maxb = max(len(q.pages) for q in self.seqs)
        bt = torch.zeros(len(sessions), maxb, dtype=torch.int32)
        for s, q in enumerate(self.seqs):
            bt[s, :len(q.pages)] = torch.tensor(q.pages, dtype=torch.int32)
        self.bt = bt.to(dev)
        self.items = torch.tensor(items, dtype=torch.int32).to(dev)
        self.nvis = torch.tensor(nvis, dtype=torch.int32).to(dev)
        self.q = torch.randn(t, H * hd, generator=g).to(dev)
        self.scale = hd ** -0.5
        self.ref = self._reference(nvis)

    def _reference(self, nvis):
        """float64 softmax(q K^T * scale) V per token and head over the session's first tok_nvis keys."""
        H, KVH, hd = self.H, self.KVH, self.hd
        G = H // KVH
        out = torch.zeros(self.T, H * hd, dtype=torch.float64)
        t = 0
        for s, (L, tn) in enumerate(self.sessions):
            pages = torch.tensor(self.seqs[s].pages, dtype=torch.long, device=self.dev)
            K = self.p32.k[0][pages].permute(1, 0, 2, 3).reshape(KVH, -1, hd).double().cpu()
            V = self.p32.v[0][pages].permute(1, 0, 2, 3).reshape(KVH, -1, hd).double().cpu()
            for i in range(tn):
                nv = nvis[t]
                qt = self.q[t].double().cpu().view(KVH, G, hd)
                sc = torch.einsum("kgd,kjd->kgj", qt, K[:, :nv]) * self.scale
                out[t] = torch.einsum("kgj,kjd->kgd", torch.softmax(sc, -1), V[:, :nv]).reshape(-1)
                t += 1
        return out

    def launch(self, pool, ns, kps, tickets, items=True, opack=None):
        H, KVH, hd, T, dev = self.H, self.KVH, self.hd, self.T, self.dev
        out = torch.full((T, H * hd), float("nan"), device=dev)
        part_ml = torch.empty(T * H * ns * 2, device=dev) if ns > 1 else None
        part_o = torch.empty(T * H * ns * hd, device=dev) if ns > 1 else None
        tk = torch.zeros(self.n_items * KVH, dtype=torch.int32, device=dev) if tickets else None
        scales = dict(kscale=pool.ks[0], vscale=pool.vs[0]) if pool.fp8 else {}
        ops.attention(self.q, T, self.items if items else None, self.n_items, self.max_rows, self.nvis, self.bt, PS,
                      pool.k[0], pool.v[0], H, KVH, hd, self.scale, ns, part_ml, part_o, out, tickets=tk,
                      keys_per_split=kps, opack=opack, **scales)
        torch.cuda.synchronize()
        if tk is not None:
            assert int(tk.abs().sum()) == 0
        return out

    def check(self, ns, kps, tickets, items=True, pack=False, kind=None, what=""):
        """The launch on the three pools: equal outputs (and packed copies), the expected kernel family and entry, all
        within ATOL of float64.  Prints the deviations before asserting."""
        pools = (self.p32, self.p16, self.p8)
        xps = [None] * 3
        if pack:
            xps = [ops.XPack(self.H * self.hd, self.dev, max(16, self.T)) for _ in pools]
            for xp in xps:
                xp.hi.zero_()
                xp.lo.zero_()
        outs = []
        for pool, xp in zip(pools, xps):
            ops.launch_counts_reset()
            ops.kv8_launch_counts_reset()
            outs.append(self.launch(pool, ns, kps, tickets, items, xp))
            c = ops.launch_counts()
            assert c[kind] == 1 and sum(c[k] for k in FAMILIES) == 1, c
            assert c["attn_opack"] == (1 if pack else 0), c
            assert ops.kv8_launch_counts() == {"kv8_append": 0, "kv8_attention": 1 if pool.fp8 else 0}
        o32, o16, o8 = outs
        d = [float((o.cpu().double() - self.ref).abs().max()) for o in outs]
        print(f"[kv e4m3 attn] {what} ns {ns} kps {kps} tickets {tickets} items {items}: |fp32 pool - f64| {d[0]:.2e}, "
              f"|bf16 pool - f64| {d[1]:.2e}, |e4m3 pool - f64| {d[2]:.2e}, e4m3 != bf16 in {int((o8 != o16).sum())}, "
              f"e4m3 != fp32 in {int((o8 != o32).sum())} elements")
        assert not any(bool(torch.isnan(o).any()) for o in outs), what
        assert torch.equal(o8, o16), what
        assert torch.equal(o8, o32), what
        if pack:
            for xp in xps[:2]:
                assert torch.equal(xps[2].hi.view(torch.int16), xp.hi.view(torch.int16)), what
                assert torch.equal(xps[2].lo.view(torch.int16), xp.lo.view(torch.int16)), what
            assert int(xps[2].hi.view(torch.int16).ne(0).sum()) > 0
        assert max(d) <= ATOL, (what, d)


_cases = {}


def _case(dev, H, KVH, hd, sessions, seed):
    key = (H, KVH, hd, tuple(sessions))
    if key not in _cases:
        _cases[key] = Case(dev, H, KVH, hd, sessions, seed)
    return _cases[key]


# (nsplit, keys per split, tickets): one split; the in-launch merge with an empty split slot (300 keys use 3 of 4);
# static splits merged by k_attn_combine
SPLITS = [(1, 128, True), (4, 128, True), (3, 128, False)]


@pytest.mark.parametrize("ns,kps,tickets", SPLITS)
@pytest.mark.parametrize("L", [1, 17, 128, 129, 300])
def test_multi_row_two_tokens_per_item(dev, L, ns, kps, tickets):
    """14 rows per item (2 tokens x 7 query heads per kv head) on k_attn_mfma<128, 8>: 1, 2 and 3 tiles of 128 keys
    (300: the ping-pong reload), one split, ticketed splits, static splits + combine."""
    c = _case(dev, 14, 2, 128, [(L, 2), (L, 2)], 100 + L)
    c.check(ns, kps, tickets, pack=tickets, kind="attn_mfma", what=f"2 tokens x {L} keys")


@pytest.mark.parametrize("ns,kps,tickets", SPLITS)
def test_ragged_item_table(dev, ns, kps, tickets):
    """3 sessions of 1 / 2 / 2 tokens with different key counts through the item table."""
    c = _case(dev, 14, 2, 128, [(40, 1), (150, 2), (300, 2)], 7)
    c.check(ns, kps, tickets, pack=tickets, kind="attn_mfma", what="ragged items")


@pytest.mark.parametrize("ns,kps,tickets", SPLITS)
def test_uniform_batch_without_item_table(dev, ns, kps, tickets):
    """items = NULL: 3 sessions of 2 tokens, item b = sequence b."""
    c = _case(dev, 14, 2, 128, [(90, 2), (200, 2), (131, 2)], 8)
    c.check(ns, kps, tickets, items=False, pack=tickets, kind="attn_mfma", what="uniform, items NULL")


@pytest.mark.parametrize("ns,kps,tickets", SPLITS)
def test_two_row_tiles(dev, ns, kps, tickets):
    """4 tokens per item (28 rows): k_attn_mfma<128, 8, 2> at 200 keys."""
    c = _case(dev, 14, 2, 128, [(200, 4), (200, 4)], 9)
    assert c.max_rows == 28
    c.check(ns, kps, tickets, pack=tickets, kind="attn_mfma", what="28 rows x 200 keys")


@pytest.mark.parametrize("ns,kps,tickets", SPLITS)
@pytest.mark.parametrize("H,KVH,hd,tn", [(4, 4, 64, 3), (4, 2, 32, 2)])
def test_four_wave_kernels(dev, H, KVH, hd, tn, ns, kps, tickets):
    """k_attn_mfma<64> and <32> (64-key tiles; head_dim 32 stages V in 8-byte pieces) at 70 keys: two tiles."""
    c = _case(dev, H, KVH, hd, [(70, tn), (70, tn)], 10 + hd)
    c.check(ns, 64 if ns > 1 else kps, tickets, pack=tickets, kind="attn_mfma", what=f"hd {hd}")


GQA_KEYS = [1, 224, 225, 448, 449]   # 224 / 225: the prefetched-V boundary of the single-row body; 448 / 449: its
                                     # crossover to the multi-row body (GQA_DEC_KEYS), both kept for the FP8 cache


@pytest.mark.parametrize("ns,kps", [(1, 128), (16, 128)])
def test_gqa_decode_one_token_per_session(dev, ns, kps):
    """k_attn_gqa_decode<128>: one token per session, the single-row body up to 448 keys and the multi-row body beyond,
    in one launch; eager (one split) and with tickets and 16 split slots."""
    c = _case(dev, 14, 2, 128, [(L, 1) for L in GQA_KEYS], 11)
    assert c.max_rows == 7 and c.T == c.n_items == len(GQA_KEYS)
    c.check(ns, kps, True, pack=True, kind="attn_gqa_decode", what=f"gqa decode {GQA_KEYS}")
    c.check(ns, kps, True, items=False, pack=True, kind="attn_gqa_decode", what=f"gqa decode {GQA_KEYS}, items NULL")


def test_forms_without_an_fp8_kernel_are_refused(dev):
    """On an FP8 pool the 2-wave form (tickets with keys_per_split 32 at head_dim 128) and the single-row decode form
    (one query row per item: H == KVH) return an error that names the entry and the form and launch nothing; the same
    calls on the fp32 pool run."""
    c = _case(dev, 14, 2, 128, [(40, 1), (150, 2), (300, 2)], 7)
    ops.launch_counts_reset()
    ops.kv8_launch_counts_reset()
    with pytest.raises(RuntimeError, match="fo_attention_kv8: .*2-wave form"):
        c.launch(c.p8, 4, 32, True)
    assert sum(ops.launch_counts().values()) == 0 and not any(ops.kv8_launch_counts().values())
    out = c.launch(c.p32, 4, 32, True)   # the fp32 pool takes that form
    assert float((out.cpu().double() - c.ref).abs().max()) <= ATOL
    d = _case(dev, 4, 4, 64, [(100, 1), (33, 1)], 12)
    assert d.max_rows == 1
    ops.launch_counts_reset()
    with pytest.raises(RuntimeError, match="fo_attention_kv8: .*single-row decode form"):
        d.launch(d.p8, 1, 128, False)
    assert sum(ops.launch_counts().values()) == 0 and not any(ops.kv8_launch_counts().values())
    ops.launch_counts_reset()
    out = d.launch(d.p32, 1, 128, False)
    assert ops.launch_counts()["attn_decode"] == 1
    assert float((out.cpu().double() - d.ref).abs().max()) <= ATOL
