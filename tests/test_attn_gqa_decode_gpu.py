"""fo_attention's one-token GQA launch at head_dim 128 (k_attn_gqa_decode: the Qwen2 text step) against a float64
reference: an item of at most GQA_DEC_KEYS visible keys takes the single-row fp32 body (one query head per split
slot, stored directly), a longer one the multi-row split body with the in-launch merge; the choice is made per item
on the device, so one captured launch serves a context as it grows across the threshold.

Every session is a fork of a shared 37-key prefix (a partial page shared copy-on-write), cut back or extended to its
context.  Tolerances: items on the single-row path atol 1e-5 / rtol 1e-5 (test_attn_gpu's fp32 decode bound), items
on the split path atol 2e-5 / rtol 1e-4 (its MFMA bound)."""
import math
import os
import re

import pytest
import torch

from fo import _lib, ops
from fo.kv import BatchMeta, KVPool, KVSeq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD, PS, B = 128, 16, 8
SPLITS = [(1, 128), (3, 64), (16, 128), (16, 256)]   # (nsplit, keys per split), all with tickets


def _gqa_dec_keys():
    """The threshold as the kernel source states it."""
    with open(os.path.join(ROOT, "freeze-omni_amd", "csrc", "fo_attn.hip")) as f:
        return int(re.search(r"constexpr int GQA_DEC_KEYS = (\d+);", f.read()).group(1))


GDK = _gqa_dec_keys()
CONTEXTS = [1, 15, 16, 17, 129, 200, GDK - 1, GDK, GDK + 1, 1200]
# the ten contexts in two ragged batches of 8 (item-table form), short and long items side by side in one launch
RAGGED = {"a": [1, 15, 16, 17, 129, 200, GDK - 1, GDK], "b": [GDK + 1, 1200, GDK, 200, 17, 1, GDK - 1, 129]}


def _reference(q, pool, seqs, meta_host, H, KVH, hd, scale):
    """tests/test_attn_gpu.py::_reference (float64 softmax(q K^T * scale) V per token and head over the session's
    first tok_nvis keys, query head h on kv head h // G), with a session's pages gathered in one indexing operation
    instead of key by key.  q [T, H*hd]; meta_host: list of (seq, tok_nvis) per token."""
    out = torch.zeros(len(meta_host), H * hd, dtype=torch.float64)
    G = H // KVH
    P = pool.PS
    for t, (s, nv) in enumerate(meta_host):
        pages = torch.tensor(seqs[s].pages[:(nv + P - 1) // P], dtype=torch.long, device=pool.k.device)
        K = pool.k[0][pages].permute(1, 0, 2, 3).reshape(KVH, -1, hd)[:, :nv].double().cpu()
        V = pool.v[0][pages].permute(1, 0, 2, 3).reshape(KVH, -1, hd)[:, :nv].double().cpu()
        qt = q[t].double().cpu().view(KVH, G, hd)
        sc = torch.einsum("kgd,kjd->kgj", qt, K) * scale
        out[t] = torch.einsum("kgj,kjd->kgd", torch.softmax(sc, -1), V).reshape(-1)
    return out


_pools, _cases = {}, {}


def _pool(dev, KVH):
    """One randomly filled pool per kv head count, shared by every case; never written after this except by the
    growing-context test, which owns its sessions' pages."""
    if KVH not in _pools:
        g = torch.Generator().manual_seed(1000 + KVH)
        pool = KVPool(1, KVH, HD, 3072 if KVH == 4 else 512, PS, dev)
        pool.k.copy_(torch.randn(pool.k.shape, generator=g))
        pool.v.copy_(torch.randn(pool.v.shape, generator=g))
        base = KVSeq(pool)
        BatchMeta([(base, 37, 0, True)], dev)   # the shared prefix, a partial last page
        _pools[KVH] = (pool, base)
    return _pools[KVH]


def _sessions(dev, KVH, ctxs):
    """Forks of the prefix holding ctx - 1 keys each (the step under test appends the last one)."""
    pool, base = _pool(dev, KVH)
    seqs = []
    for L in ctxs:
        s = base.fork()
        if L - 1 < 37:
            s.truncate(L - 1)
        elif L - 1 > 37:
            BatchMeta([(s, L - 1 - 37, s.length, True)], dev)
        seqs.append(s)
    return pool, seqs


def _case(dev, H, KVH, name):
    """name: 'a' / 'b' (RAGGED) or an int (8 sessions of that context).  The step's tables, q and the float64
    reference, computed once and shared by the split settings and tests; nothing in it is written afterwards."""
    key = (H, KVH, name)
    if key not in _cases:
        ctxs = RAGGED[name] if name in RAGGED else [name] * B
        pool, seqs = _sessions(dev, KVH, ctxs)
        meta = BatchMeta([(s, 1, s.length, True) for s in seqs], dev, gqa=H // KVH)
        assert meta.max_rows == H // KVH and meta.n_items == meta.T == B
        assert meta.tok_nvis.cpu().tolist() == ctxs
        g = torch.Generator().manual_seed(H * 31 + sum(ctxs))
        q = torch.randn(B, H * HD, generator=g).to(dev)
        ref = _reference(q, pool, seqs, list(enumerate(ctxs)), H, KVH, HD, 1 / math.sqrt(HD))
        _cases[key] = (pool, seqs, meta, q, ref, ctxs)
    return _cases[key]


def _buffers(dev, H, KVH, ns, T=B):
    part_ml = torch.empty(T * H * ns * 2, device=dev) if ns > 1 else None
    part_o = torch.empty(T * H * ns * HD, device=dev) if ns > 1 else None
    return part_ml, part_o, torch.zeros(T * KVH, dtype=torch.int32, device=dev)


def _launch(pool, meta, q, H, KVH, ns, kps, out, bufs, items=True, nvis=None, opack=None):
    part_ml, part_o, tickets = bufs
    ops.attention(q, meta.T, meta.items if items else None, meta.n_items, meta.max_rows,
                  meta.tok_nvis if nvis is None else nvis, meta.block_table, pool.PS, pool.k[0], pool.v[0], H, KVH, HD,
                  1 / math.sqrt(HD), ns, part_ml, part_o, out, tickets=tickets, keys_per_split=kps, opack=opack)


def _assert_close(out, ref, ctxs, what=""):
    """Per item: the single-row bound up to GQA_DEC_KEYS keys, the MFMA bound beyond.  Prints the worst deviations
    before asserting."""
    o = out.cpu().double()
    worst = [float((o[b] - ref[b]).abs().max()) for b in range(len(ctxs))]
    print(f"[gqa decode] {what} contexts {ctxs} worst abs {['%.1e' % w for w in worst]}")
    for b, L in enumerate(ctxs):
        atol, rtol = (1e-5, 1e-5) if L <= GDK else (2e-5, 1e-4)
        torch.testing.assert_close(o[b], ref[b], atol=atol, rtol=rtol, msg=lambda m: f"{what} item {b} (L = {L}): {m}")


def _counts_ok():
    c = ops.launch_counts()
    assert c["attn_gqa_decode"] == 1 and c["attn_mfma"] == 0 and c["attn_decode"] == 0, c


@pytest.mark.parametrize("ns,kps", SPLITS)
@pytest.mark.parametrize("H,KVH", [(28, 4), (8, 2)])
@pytest.mark.parametrize("name", ["a", "b"])
def test_item_table_matches_reference(dev, H, KVH, name, ns, kps):
    """Ragged contexts through the item table, launched twice (the second from the tickets the first left: zero)."""
    pool, seqs, meta, q, ref, ctxs = _case(dev, H, KVH, name)
    bufs = _buffers(dev, H, KVH, ns)
    out = torch.empty(B, H * HD, device=dev)
    for rep in range(2):
        out.fill_(float("nan"))
        ops.launch_counts_reset()
        _launch(pool, meta, q, H, KVH, ns, kps, out, bufs)
        torch.cuda.synchronize()
        _counts_ok()
        _assert_close(out, ref, ctxs, f"items {name} H {H} ns {ns} kps {kps} launch {rep}")
        assert int(bufs[2].abs().sum()) == 0


@pytest.mark.parametrize("ns,kps", SPLITS)
@pytest.mark.parametrize("L", CONTEXTS)
def test_dense_form_matches_reference(dev, L, ns, kps):
    """items = None (item b = sequence b = token b, T == n_items): 8 sessions at the same context."""
    H, KVH = 28, 4
    pool, seqs, meta, q, ref, ctxs = _case(dev, H, KVH, L)
    bufs = _buffers(dev, H, KVH, ns)
    out = torch.empty(B, H * HD, device=dev)
    for rep in range(2):
        out.fill_(float("nan"))
        ops.launch_counts_reset()
        _launch(pool, meta, q, H, KVH, ns, kps, out, bufs, items=False)
        torch.cuda.synchronize()
        _counts_ok()
        _assert_close(out, ref, ctxs, f"dense L {L} ns {ns} kps {kps} launch {rep}")
        assert int(bufs[2].abs().sum()) == 0


@pytest.mark.parametrize("H,KVH", [(28, 4), (8, 2)])
@pytest.mark.parametrize("name", ["a", "b"])
def test_short_items_do_not_depend_on_the_splits(dev, H, KVH, name):
    """Items of at most GQA_DEC_KEYS keys: bit-identical output whatever (nsplit, keys_per_split) the launch carries,
    with and without the item table -- so an eager launch and a captured graph's (16 slots of 128 keys) agree
    exactly."""
    pool, seqs, meta, q, ref, ctxs = _case(dev, H, KVH, name)
    short = [b for b, L in enumerate(ctxs) if L <= GDK]
    assert short
    outs = []
    for ns, kps in SPLITS:
        for items in (True, False):
            out = torch.full((B, H * HD), float("nan"), device=dev)
            _launch(pool, meta, q, H, KVH, ns, kps, out, _buffers(dev, H, KVH, ns), items=items)
            outs.append(out[short].clone())
    torch.cuda.synchronize()
    assert not torch.isnan(outs[0]).any()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def _packed_rows(t, K, rb):
    """tests/test_xpack_gpu.py::_check_packed_rb's view: a packed half ([K/32][row blocks][64][8]) as [16 rb, K]."""
    return t[:K * 16 * rb].view(K // 32, rb, 4, 16, 8).permute(1, 3, 0, 2, 4).reshape(rb * 16, K)


def _split(y):
    hi = y.to(torch.bfloat16)
    return hi, (y - hi.float()).to(torch.bfloat16)


@pytest.mark.parametrize("ns,kps", [(1, 128), (16, 128)])
@pytest.mark.parametrize("name", ["a", "b"])
def test_packed_output_is_the_split_of_out(dev, name, ns, kps):
    """fo_attention_set_opack armed: the packed hi / lo copy equals the bf16 split of the fp32 rows, for the items of
    both paths in one launch."""
    H, KVH = 28, 4
    pool, seqs, meta, q, ref, ctxs = _case(dev, H, KVH, name)
    xp = ops.XPack(H * HD, dev, B)
    xp.hi.zero_()
    xp.lo.zero_()
    out = torch.full((B, H * HD), float("nan"), device=dev)
    bufs = _buffers(dev, H, KVH, ns)
    ops.launch_counts_reset()
    _launch(pool, meta, q, H, KVH, ns, kps, out, bufs, opack=xp)
    torch.cuda.synchronize()
    c = ops.launch_counts()
    assert c["attn_gqa_decode"] == 1 and c["attn_opack"] == 1 and c["attn_mfma"] == 0, c
    _assert_close(out, ref, ctxs, f"packed {name} ns {ns}")
    hi, lo = _split(out)
    assert torch.equal(_packed_rows(xp.hi, H * HD, xp.rb)[:B].view(torch.int16), hi.view(torch.int16))
    assert torch.equal(_packed_rows(xp.lo, H * HD, xp.rb)[:B].view(torch.int16), lo.view(torch.int16))
    assert int(bufs[2].abs().sum()) == 0


@pytest.mark.parametrize("ns,kps", [(1, 128), (16, 128)])
def test_poison_on_the_short_path(dev, ns, kps):
    """A block table of 4 pages and one session whose tok_nvis claims 100 keys (7 pages): that item's fp32 rows and
    packed rows are NaN, nothing is read beyond the table; the other items are finite and right, tickets zero."""
    H, KVH = 28, 4
    ctxs = [5, 20, 40, 64, 33, 17, 50, 60]
    pool, seqs = _sessions(dev, KVH, ctxs)
    meta = BatchMeta([(s, 1, s.length, True) for s in seqs], dev, gqa=H // KVH)
    assert meta.block_table.shape[1] == 4
    bad = 2
    nv = meta.tok_nvis.clone()
    nv[bad] = 100
    q = torch.randn(B, H * HD, generator=torch.Generator().manual_seed(5)).to(dev)
    ref = _reference(q, pool, seqs, list(enumerate(ctxs)), H, KVH, HD, 1 / math.sqrt(HD))
    xp = ops.XPack(H * HD, dev, B)
    xp.hi.zero_()   # a stale, finite previous content
    xp.lo.zero_()
    out = torch.zeros(B, H * HD, device=dev)
    bufs = _buffers(dev, H, KVH, ns)
    ops.launch_counts_reset()
    _launch(pool, meta, q, H, KVH, ns, kps, out, bufs, nvis=nv, opack=xp)
    torch.cuda.synchronize()
    c = ops.launch_counts()
    assert c["attn_gqa_decode"] == 1 and c["attn_mfma"] == 0, c
    others = [b for b in range(B) if b != bad]
    assert torch.isnan(out[bad]).all()
    assert torch.isfinite(out[others]).all()
    _assert_close(out[others], ref[others], [ctxs[b] for b in others], f"poison ns {ns}")
    ph = _packed_rows(xp.hi, H * HD, xp.rb)[:B].float()
    pl = _packed_rows(xp.lo, H * HD, xp.rb)[:B].float()
    assert torch.isnan(ph[bad]).all() and torch.isnan(pl[bad]).all()
    hi, lo = _split(out[others])
    assert torch.equal(ph[others], hi.float()) and torch.equal(pl[others], lo.float())
    assert int(bufs[2].abs().sum()) == 0
    for s in seqs:
        s.free()


def test_static_splits_without_tickets_keep_the_multi_row_launch(dev):
    """tickets = None, nsplit = 3: k_attn_combine follows and would overwrite a directly stored row."""
    H, KVH = 28, 4
    pool, seqs, meta, q, ref, ctxs = _case(dev, H, KVH, "a")
    ns = 3
    out = torch.full((B, H * HD), float("nan"), device=dev)
    ops.launch_counts_reset()
    ops.attention(q, B, meta.items, meta.n_items, meta.max_rows, meta.tok_nvis, meta.block_table, pool.PS, pool.k[0],
                  pool.v[0], H, KVH, HD, 1 / math.sqrt(HD), ns, torch.empty(B * H * ns * 2, device=dev),
                  torch.empty(B * H * ns * HD, device=dev), out)
    torch.cuda.synchronize()
    c = ops.launch_counts()
    assert c["attn_mfma"] == 1 and c["attn_gqa_decode"] == 0, c
    torch.testing.assert_close(out.cpu().double(), ref, atol=2e-5, rtol=1e-4)


def test_one_head_per_kv_head_still_takes_the_decode_kernel(dev):
    """(14, 14, 64), one token per session: k_attn_decode, as before."""
    H = KVH = 14
    hd = 64
    g = torch.Generator().manual_seed(64)
    pool = KVPool(1, KVH, hd, 64, PS, dev)
    pool.k.copy_(torch.randn(pool.k.shape, generator=g))
    pool.v.copy_(torch.randn(pool.v.shape, generator=g))
    seqs = [KVSeq(pool) for _ in range(4)]
    lens = [1, 17, 100, 333]
    for s, n in zip(seqs, lens):
        if n > 1:
            BatchMeta([(s, n - 1, 0, True)], dev)
    meta = BatchMeta([(s, 1, s.length, True) for s in seqs], dev, gqa=1)
    q = torch.randn(4, H * hd, generator=g).to(dev)
    out = torch.full((4, H * hd), float("nan"), device=dev)
    ops.launch_counts_reset()
    ops.attention(q, 4, meta.items, meta.n_items, meta.max_rows, meta.tok_nvis, meta.block_table, pool.PS, pool.k[0],
                  pool.v[0], H, KVH, hd, 1 / math.sqrt(hd), 1, None, None, out)
    torch.cuda.synchronize()
    c = ops.launch_counts()
    assert c["attn_decode"] == 1 and c["attn_gqa_decode"] == 0 and c["attn_mfma"] == 0, c
    ref = _reference(q, pool, seqs, list(enumerate(lens)), H, KVH, hd, 1 / math.sqrt(hd))
    torch.testing.assert_close(out.cpu().double(), ref, atol=1e-5, rtol=1e-5)


def test_two_tokens_per_session_keep_the_multi_row_launch(dev):
    H, KVH = 28, 4
    ctxs = [3, 40, 150, 300, 17, 64, 129, GDK]
    pool, seqs = _sessions(dev, KVH, [L - 1 for L in ctxs])   # L - 2 keys, then the step's two tokens
    meta = BatchMeta([(s, 2, s.length, True) for s in seqs], dev, gqa=H // KVH)
    T = meta.T
    assert T == 16 and meta.max_rows == 14
    q = torch.randn(T, H * HD, generator=torch.Generator().manual_seed(9)).to(dev)
    host = list(zip(meta.tok_seq.cpu().tolist(), meta.tok_nvis.cpu().tolist()))
    ref = _reference(q, pool, seqs, host, H, KVH, HD, 1 / math.sqrt(HD))
    ns = 16
    bufs = _buffers(dev, H, KVH, ns, T)
    out = torch.full((T, H * HD), float("nan"), device=dev)
    ops.launch_counts_reset()
    _launch(pool, meta, q, H, KVH, ns, 128, out, bufs)
    torch.cuda.synchronize()
    c = ops.launch_counts()
    assert c["attn_mfma"] == 1 and c["attn_gqa_decode"] == 0, c
    torch.testing.assert_close(out.cpu().double(), ref, atol=2e-5, rtol=1e-4)
    assert int(bufs[2].abs().sum()) == 0
    for s in seqs:
        s.free()


def test_one_captured_launch_serves_a_growing_context(dev):
    """One launch captured at a capacity of 2048 keys (16 slots of 128 keys, a 128-page block table) and replayed
    while each session's tok_nvis, appended key and block table advance from GQA_DEC_KEYS - 3 to GQA_DEC_KEYS + 3,
    the sessions staggered so that one replay holds items of both paths; every replay against float64, and against an
    eager one-split launch bit for bit on the short items."""
    from fo.engine import ListenGraph
    H, KVH = 28, 4
    G = H // KVH
    scale = 1 / math.sqrt(HD)
    stagger = [0, 1, 2, 0, -1, 1, -2, 0]
    start = [GDK - 3 + d for d in stagger]
    pool, seqs = _sessions(dev, KVH, start)          # start - 1 keys each
    maxb = 2048 // PS
    g = torch.Generator().manual_seed(77)
    main = ops.engine_stream(dev)
    nvis = torch.zeros(B, dtype=torch.int32, device=dev)
    bt = torch.zeros(B, maxb, dtype=torch.int32, device=dev)
    q = torch.empty(B, H * HD, device=dev)
    out = torch.empty(B, H * HD, device=dev)
    ns = ops.attn_nsplit(2048, B, KVH)
    assert ns == 16
    bufs = _buffers(dev, H, KVH, ns)
    with torch.cuda.stream(main):
        ops.Runtime.get(dev)

    def body():
        ops.attention(q, B, None, B, G, nvis, bt, PS, pool.k[0], pool.v[0], H, KVH, HD, scale, ns, bufs[0], bufs[1],
                      out, tickets=bufs[2], keys_per_split=128)

    nvis.fill_(1)
    torch.cuda.synchronize()
    with torch.cuda.stream(main):
        body()   # the kernel is loaded before the capture
    torch.cuda.synchronize()
    ops.launch_counts_reset()
    ex = ListenGraph._capture(main, body)
    try:
        c = ops.launch_counts()
        assert c["attn_gqa_decode"] == 1 and c["attn_mfma"] == 0, c
        seen = set()
        for step in range(7):
            # the step's token: a page when the context crosses one, a fresh key / value row in its slot
            slots = []
            for s in seqs:
                s.reserve(s.length + 1)
                slots.append(s.slot(s.length))
                s.length += 1
            ctxs = [s.length for s in seqs]
            hb = torch.zeros(B, maxb, dtype=torch.int32)
            for b, s in enumerate(seqs):
                hb[b, :len(s.pages)] = torch.tensor(s.pages, dtype=torch.int32)
            sl = torch.tensor(slots, dtype=torch.long, device=dev)
            with torch.cuda.stream(main):
                # the cache rows are [page][kv head][slot][hd]
                kn = torch.randn(B, KVH, HD, generator=g).to(dev)
                vn = torch.randn(B, KVH, HD, generator=g).to(dev)
                pool.k[0][sl // PS, :, sl % PS] = kn
                pool.v[0][sl // PS, :, sl % PS] = vn
                q.copy_(torch.randn(B, H * HD, generator=g).to(dev))
                nvis.copy_(torch.tensor(ctxs, dtype=torch.int32).to(dev))
                bt.copy_(hb.to(dev))
                out.fill_(float("nan"))
                _lib.call("fo_graph_launch", ex, main.cuda_stream)
            torch.cuda.synchronize()
            ref = _reference(q, pool, seqs, list(enumerate(ctxs)), H, KVH, HD, scale)
            _assert_close(out, ref, ctxs, f"replay {step}")
            assert int(bufs[2].abs().sum()) == 0
            short = [b for b, L in enumerate(ctxs) if L <= GDK]
            seen.update("short" if L <= GDK else "long" for L in ctxs)
            if short:
                eager = torch.full((B, H * HD), float("nan"), device=dev)
                ops.attention(q, B, None, B, G, nvis, bt, PS, pool.k[0], pool.v[0], H, KVH, HD, scale, 1, None, None,
                              eager, tickets=torch.zeros(B * KVH, dtype=torch.int32, device=dev), keys_per_split=256)
                torch.cuda.synchronize()
                assert torch.equal(eager[short], out[short])
        assert seen == {"short", "long"}
        assert [s.length for s in seqs] == [GDK + 3 + d for d in stagger]
    finally:
        _lib.call("fo_graph_destroy", ex)
        for s in seqs:
            s.free()
