"""fo_attention on a bf16 paged KV against the same call on an fp32 pool that holds the same values.

A K or V that is a bf16 value splits into hi = value, lo = 0, so the fp32 kernels' MFMA against the low half adds an
exact zero; the bf16 kernels read 2-byte elements and drop that MFMA, everything else in the same order.  The two
results must therefore be EQUAL (torch.equal on the floats; +0 and -0 compare equal), for every kernel form: the
8-wave multi-row kernel with one split, the in-launch merge and the combine launch, its two-row-tile form, the 4-wave
kernels at head_dim 64 and 32, the one-token GQA launch on both of its bodies, and the single-row decode kernel.  Both
results are also held to the project's attention tolerance, 2e-5 abs, against a float64 softmax attention on those
values.

Inputs: q, K, V ~ N(0, 1), K / V rounded to bf16, scale = hd^-0.5 (scores within about +-16: no term is denormal).
Pages are dealt in a shuffled order; both pools are pre-filled with NaN, so a read outside a session's keys shows.
"""
import math
import random
from types import SimpleNamespace

import pytest
import torch

from fo import ops
from fo.kv import KVPool, KVSeq

pytestmark = pytest.mark.gpu
PS = 16
ATOL = 2e-5   # the project's attention tolerance (tests/test_attn_gpu.py's MFMA bound)


class Case:
    """sessions: [(keys, tokens)]: each session holds `keys` keys and the launch carries its last `tokens` tokens,
    causal (token i of tn sees keys - (tn - 1 - i), at least 1: at one key both tokens of an item see it).  One work
    item per session.  Builds both pools, the launch tables, q and the float64 reference once."""

    def __init__(self, dev, H, KVH, hd, sessions, seed):
        g = torch.Generator().manual_seed(seed)
        n_pages = sum((L + PS - 1) // PS for L, _ in sessions) + 5
        self.dev, self.H, self.KVH, self.hd, self.sessions = dev, H, KVH, hd, sessions
        self.p32 = KVPool(1, KVH, hd, n_pages, PS, dev)
        self.p16 = KVPool(1, KVH, hd, n_pages, PS, dev, dtype=torch.bfloat16)
        assert self.p16.k.dtype == torch.bfloat16 and self.p16.k.shape == self.p32.k.shape
        random.Random(seed).shuffle(self.p32.free)   # pages dealt in a shuffled, non-contiguous order
        for p in (self.p32, self.p16):
            p.k.fill_(float("nan"))
            p.v.fill_(float("nan"))
        self.seqs, items, nvis, t = [], [], [], 0
        for s, (L, tn) in enumerate(sessions):
            seq = KVSeq(self.p32)
            seq.reserve(L)
            seq.length = L
            self.seqs.append(seq)
            sl = torch.tensor([seq.slot(p) for p in range(L)], dtype=torch.long, device=dev)
            for name in ("k", "v"):
                x = torch.randn(L, KVH, hd, generator=g).to(torch.bfloat16).to(dev)
                getattr(self.p16, name)[0][sl // PS, :, sl % PS] = x
                getattr(self.p32, name)[0][sl // PS, :, sl % PS] = x.float()
            items += [s, t, tn]
            nvis += [max(1, L - (tn - 1 - i)) for i in range(tn)]
            t += tn
        self.T, self.n_items = t, len(sessions)
        self.max_rows = max(tn for _, tn in sessions) * (H // KVH)
        self.uniform = len({tn for _, tn in sessions}) == 1
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
        ops.attention(self.q, T, self.items if items else None, self.n_items, self.max_rows, self.nvis, self.bt, PS,
                      pool.k[0], pool.v[0], H, KVH, hd, self.scale, ns, part_ml, part_o, out, tickets=tk,
                      keys_per_split=kps, opack=opack)
        torch.cuda.synchronize()
        if tk is not None:
            assert int(tk.abs().sum()) == 0
        return out

    def check(self, ns, kps, tickets, items=True, pack=False, kind=None, what=""):
        """The launch on both pools: equal outputs (and packed copies), the expected kernel family, both within ATOL
        of float64.  Prints the deviations before asserting."""
        xps = [None, None]
        if pack:
            xps = [ops.XPack(self.H * self.hd, self.dev, max(16, self.T)) for _ in range(2)]
            for xp in xps:
                xp.hi.zero_()
                xp.lo.zero_()
        outs = []
        for pool, xp in zip((self.p32, self.p16), xps):
            ops.launch_counts_reset()
            outs.append(self.launch(pool, ns, kps, tickets, items, xp))
            c = ops.launch_counts()
            if kind:
                assert c[kind] == 1 and sum(c[k] for k in ("attn_mfma", "attn_decode", "attn_gqa_decode")) == 1, c
            assert c["attn_opack"] == (1 if pack else 0), c
        o32, o16 = outs
        d32 = float((o32.cpu().double() - self.ref).abs().max())
        d16 = float((o16.cpu().double() - self.ref).abs().max())
        print(f"[kv bf16 attn] {what} ns {ns} kps {kps} tickets {tickets} items {items}: |fp32 pool - f64| {d32:.2e}, "
              f"|bf16 pool - f64| {d16:.2e}, differing elements {int((o32 != o16).sum())}")
        assert not torch.isnan(o32).any() and not torch.isnan(o16).any(), what
        assert torch.equal(o16, o32), what
        if pack:
            assert torch.equal(xps[0].hi.view(torch.int16), xps[1].hi.view(torch.int16)), what
            assert torch.equal(xps[0].lo.view(torch.int16), xps[1].lo.view(torch.int16)), what
            assert int(xps[1].hi.view(torch.int16).ne(0).sum()) > 0
        assert d32 <= ATOL and d16 <= ATOL, (what, d32, d16)


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
    """k_attn_mfma<64> and <32> (64-key tiles) at 70 keys: two tiles."""
    c = _case(dev, H, KVH, hd, [(70, tn), (70, tn)], 10 + hd)
    c.check(ns, 64 if ns > 1 else kps, tickets, pack=tickets, kind="attn_mfma", what=f"hd {hd}")


GQA_KEYS = [1, 224, 225, 448, 449]   # 224 / 225: the prefetched-V boundary of the single-row body (unchanged for bf16);
                                     # 448 / 449: its crossover to the multi-row body (GQA_DEC_KEYS, kept for bf16)


@pytest.mark.parametrize("ns,kps", [(1, 128), (16, 128)])
@pytest.mark.parametrize("items", [True, False])
def test_gqa_decode_one_token_per_session(dev, ns, kps, items):
    """k_attn_gqa_decode<128>: one token per session, the single-row body up to 448 keys and the multi-row body beyond,
    in one launch; eager (one split) and with tickets and 16 split slots."""
    c = _case(dev, 14, 2, 128, [(L, 1) for L in GQA_KEYS], 11)
    assert c.max_rows == 7 and c.T == c.n_items == len(GQA_KEYS)
    c.check(ns, kps, True, items=items, pack=True, kind="attn_gqa_decode", what=f"gqa decode {GQA_KEYS}")


def test_single_row_decode_kernel(dev):
    """k_attn_decode<64> (H = KVH = 4, one row per item) at 100 keys."""
    c = _case(dev, 4, 4, 64, [(100, 1), (33, 1)], 12)
    assert c.max_rows == 1
    c.check(1, 128, False, kind="attn_decode", what="decode hd 64")
    c.check(1, 128, False, items=False, pack=True, kind="attn_decode", what="decode hd 64, items NULL, packed")


def test_forms_without_a_bf16_kernel_are_refused(dev):
    """On a bf16 pool fo_attention_o and the 2-wave form (tickets with keys_per_split 32 at head_dim 128) return an
    error that names the form and launch nothing; the same calls' fp32 pool is not refused for its layout."""
    c = _case(dev, 14, 2, 128, [(40, 1), (150, 2), (300, 2)], 7)
    ops.launch_counts_reset()
    with pytest.raises(RuntimeError, match="2-wave form"):
        c.launch(c.p16, 4, 32, True)
    assert sum(ops.launch_counts().values()) == 0
    out = c.launch(c.p32, 4, 32, True)   # the fp32 pool takes that form
    assert float((out.cpu().double() - c.ref).abs().max()) <= ATOL
    # the fused decode attention + o projection: refused before any argument is used
    d = _case(dev, 4, 4, 64, [(100, 1), (33, 1)], 12)
    z = torch.zeros(64, device=dev)
    zi = torch.zeros(8, dtype=torch.int32, device=dev)
    wo = SimpleNamespace(packed=z, N=1)
    stats = SimpleNamespace(buf=z, groups=0)
    ops.launch_counts_reset()
    with pytest.raises(RuntimeError, match="fo_attention_o.*fp32 cache only"):
        ops.attention_o(d.q, d.T, None, d.nvis, d.bt, PS, d.p16.k[0], d.p16.v[0], 4, 64, d.scale, wo, z, zi, z, z, z,
                        stats)
    torch.cuda.synchronize()
    assert sum(ops.launch_counts().values()) == 0 and stats.groups == 0
    with pytest.raises(ValueError, match="both be fp32 or both bf16"):
        ops.kv_bytes(c.p16.k[0], c.p32.v[0])
