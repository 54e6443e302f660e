"""llm_kv="bf16" through the engines: an engine whose Qwen2 pool holds bf16 elements against an engine
with the default fp32 pool under fo_set_kv_bf16(1), which holds the same values widened.  The two compute the same
thing bit for bit, so everything is compared with torch.equal / ==: hidden rows, state probabilities, drawn ids,
context lengths and page lists.  Nothing here compares against the fp32 default with a tolerance (the option's
distance from the default is documented in DESIGN, not asserted), and no golden's expected outputs are read: the
real-geometry part takes only the input embeddings of tests/golden/real_qwen2_t2.npz.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")


class _rounded:
    """fo_set_kv_bf16(1) for the block (an fp32 pool then holds bf16 values); the previous value is restored."""

    def __enter__(self):
        from fo import _lib
        self.lib = _lib.load()
        self.prev = self.lib.fo_set_kv_bf16(1)
        assert self.prev in (0, 1)

    def __exit__(self, *exc):
        assert self.lib.fo_set_kv_bf16(self.prev) == 1
        return False


# ------------------------------------------------------------------ two layers at real geometry
@pytest.fixture(scope="module")
def pair(dev):
    """(A: fp32 pool, B: kv_dtype="bf16"), built as tests/test_real_qwen2_gpu.py builds its engine, on one source."""
    from fo.llm import LLMEngine
    from fo.weights import SynthSource
    from oracle import configs
    from oracle.params import all_shapes
    cfg = configs.get("real")
    cfg["llm"]["num_hidden_layers"] = 2
    src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
    A = LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16)
    B = LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16, kv_dtype="bf16")
    assert (A.D, A.H, A.KVH, A.hd) == (3584, 28, 4, 128)
    assert A.pool.k.dtype == torch.float32 and B.pool.k.dtype == torch.bfloat16 and B.kv_dtype == "bf16"
    with pytest.raises(ValueError):
        LLMEngine(src, cfg["llm"], dev, kv_tokens=64, page_size=16, kv_dtype="fp16")
    return A, B


def _golden_flow(llm, dev, gold):
    """The golden's inputs: the 128-row prefill, two 2-row chunks, then three text steps from a captured TextGraph fed
    its own greedy ids.  Returns everything the steps hand back, and the contexts' lengths and page lists."""
    from fo import ops
    from fo.engine import TextGraph
    B = 8
    rows0 = gold["rows0"].tolist()
    seqs = [llm.new_seq() for _ in range(B)]
    out = {}
    try:
        for s, rows in ((0, rows0), (1, [2] * B), (2, [2] * B)):
            x = torch.from_numpy(gold[f"emb{s}"].astype(np.float32)).to(dev)
            h, bm = llm.forward(x, [(q, r) for q, r in zip(seqs, rows)])
            out[f"hid{s}"] = h[:sum(rows)].clone()
            out[f"probs{s}"] = llm.state_probs(h, bm.last_rows_host).clone()
        lg = llm.logits(h, bm.last_rows_host)
        ids = torch.empty(B, dtype=torch.int32, device=dev)
        ops.sample(lg, llm.V, ids, torch.ones(B, dtype=torch.int32, device=dev))
        feed = ids.cpu().tolist()
        out["ids2"] = feed
        g = TextGraph(SimpleNamespace(device=dev, llm=llm), B, 2048, 1, 0.0, 1.0, 0)
        try:
            for s in (3, 4, 5):
                feed, hid = g.run([(q, [t]) for q, t in zip(seqs, feed)])
                out[f"ids{s}"] = list(feed)
                out[f"hid{s}"] = hid.clone()
                out[f"probs{s}"] = llm.state_probs(hid, list(range(B))).clone()
        finally:
            g.destroy()
        out["lengths"] = [q.length for q in seqs]
        out["pages"] = [list(q.pages) for q in seqs]
        assert out["lengths"] == [r + 7 for r in rows0]
    finally:
        for q in seqs:
            q.free()
    assert llm.pool.pages_in_use() == 0
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            d = int((a[k] != b[k]).sum())
            print(f"[kv bf16 engine] {what} {k}: {a[k].numel()} elements, {d} differ")
            assert not torch.isnan(a[k]).any(), (what, k)
            assert torch.equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


@pytest.mark.gpu
def test_real_geometry_prefill_chunks_and_text_graph(dev, pair):
    from goldenio import load_golden
    gold = load_golden("real_qwen2_t2.npz")
    A, B = pair
    assert B.pool.bytes_per_token * 2 == A.pool.bytes_per_token == 2 * 4 * 128 * 4 * 2
    assert 2 * (B.pool.k.numel() * B.pool.k.element_size() + B.pool.v.numel() * B.pool.v.element_size()) == \
        A.pool.k.numel() * A.pool.k.element_size() + A.pool.v.numel() * A.pool.v.element_size()
    assert A.pool.n_pages == B.pool.n_pages
    with _rounded():
        a = _golden_flow(A, dev, gold)
        b = _golden_flow(B, dev, gold)
    _same(a, b, "golden flow")


def _fork_flow(llm, dev, gold):
    """A 20-row prompt (a partial second page), forked twice, a different chunk appended to each fork in one forward:
    the tail page is copied on write, in the pool's own element.  Returns the forks' rows and the parent's keys."""
    x0 = torch.from_numpy(gold["emb0"][:20].astype(np.float32)).to(dev)
    xa = torch.from_numpy(gold["emb0"][20:23].astype(np.float32)).to(dev)
    xb = torch.from_numpy(gold["emb0"][40:45].astype(np.float32)).to(dev)
    pool = llm.pool
    parent = llm.new_seq()
    out = {}
    forks = []
    try:
        h, _ = llm.forward(x0, [(parent, 20)])
        out["prompt"] = h[:20].clone()
        pages = torch.tensor(parent.pages, dtype=torch.long, device=dev)
        before = (pool.k[:, pages].clone(), pool.v[:, pages].clone())
        forks = [parent.fork(), parent.fork()]
        assert forks[0].pages == parent.pages and int(pool.ref[parent.pages[1]]) == 3
        h, bm = llm.forward(torch.cat([xa, xb]), [(forks[0], 3), (forks[1], 5)])
        out["forks"] = h[:8].clone()
        out["probs"] = llm.state_probs(h, bm.last_rows_host).clone()
        # the partial tail page was copied for each fork, the full first page is still shared
        assert forks[0].pages[0] == forks[1].pages[0] == parent.pages[0]
        assert len({forks[0].pages[1], forks[1].pages[1], parent.pages[1]}) == 3
        assert torch.equal(pool.k[:, pages], before[0]) and torch.equal(pool.v[:, pages], before[1])
        for f in forks:   # the copied tail: the parent's 4 keys of that page, in the pool's element
            assert torch.equal(pool.k[:, f.pages[1], :, :4], pool.k[:, parent.pages[1], :, :4])
            assert torch.equal(pool.v[:, f.pages[1], :, :4], pool.v[:, parent.pages[1], :, :4])
        # the parent goes on from its own untouched keys
        h, _ = llm.forward(xb[:2].clone(), [(parent, 2)])
        out["parent_next"] = h[:2].clone()
        out["parent_keys"] = torch.cat([pool.k[:, pages].float(), pool.v[:, pages].float()])[..., :4, :]
        out["lengths"] = [parent.length] + [f.length for f in forks]
        out["pages"] = [list(parent.pages)] + [list(f.pages) for f in forks]
        assert out["lengths"] == [22, 23, 25]
    finally:
        for q in forks + [parent]:
            q.free()
    assert pool.pages_in_use() == 0
    return out


@pytest.mark.gpu
def test_real_geometry_copy_on_write_forks(dev, pair):
    from goldenio import load_golden
    gold = load_golden("real_qwen2_t2.npz")
    A, B = pair
    with _rounded():
        a = _fork_flow(A, dev, gold)
        b = _fork_flow(B, dev, gold)
    _same(a, b, "fork flow")


# ------------------------------------------------------------------ tiny config, the whole engine
def _tiny_flow(eng, dev):
    """System prompt, 3 sessions forked from it (the shared chat-prefix cache), listen chunks through the captured
    ListenGraph and eagerly, a grouped listen at 2 chunks per stage (5 chunks: 2 + 2 + 1), two text steps."""
    feats = torch.from_numpy(np.load(os.path.join(G, "fbank.npz"))["A_feats"]).to(dev)   # [13, 19, 80]
    n = 3
    out = {}

    def sessions():
        base = eng.system_role("<|im_start|>system\nYou are a helpful assistant.")
        return base, [base.fork() for _ in range(n)], [dict(enc_cache=None, ada_cache=None, pe_index=0) for _ in range(n)]

    def chunk(c, kvs, state):
        return [dict(identity="user", status="ipu_sl" if c == 0 else "ipu_cl", feats=feats[(c + 4 * u) % 13],
                     kv=kvs[u], **state[u]) for u in range(n)]

    for graph in (True, False):
        base, kvs, state = sessions()
        try:
            for c in range(4):
                res = eng.listen(chunk(c, kvs, state), graph=graph)
                for u, r in enumerate(res):
                    state[u] = dict(enc_cache=r["enc_cache"], ada_cache=r["ada_cache"], pe_index=r["pe_index"])
                out[f"listen g{int(graph)} c{c} probs"] = [(r["probs"]["state_1"], r["probs"]["state_2"]) for r in res]
                out[f"listen g{int(graph)} c{c} rows"] = torch.stack([r["hidden_row"][0][r["hidden_row"][1]] for r in res])
            if graph:
                feed = [[7, 12, 99], [300, 45, 100]]
                for j, ids in enumerate(feed):
                    got, hid = eng.text_step([(kv, [t]) for kv, t in zip(kvs, ids)])
                    out[f"text {j} ids"] = list(got)
                    out[f"text {j} hid"] = hid.clone()
                got, hid = eng.text_step([(kv, [t, t + 1]) for kv, t in zip(kvs, feed[0])], graph=False)
                out["text eager ids"], out["text eager hid"] = list(got), hid.clone()
            out[f"listen g{int(graph)} lengths"] = [kv.length for kv in kvs]
        finally:
            for kv in kvs + [base]:
                kv.free()
    assert len(eng._lgraphs) >= 1 and len(eng._tgraphs) >= 1   # the captured paths really ran
    # the grouped listen (ListenGraph(chunks=C)), the bench's order
    base, kvs, state = sessions()
    try:
        pipe = eng.listen_pipe(2)
        k = 0

        def record(groups):
            nonlocal k
            for res in groups or []:
                out[f"group {k} probs"] = [(r["probs"]["state_1"], r["probs"]["state_2"]) for r in res]
                out[f"group {k} rows"] = torch.stack([r["hidden_row"][0][r["hidden_row"][1]].clone() for r in res])
                k += 1

        for c in range(5):
            items = chunk(c, kvs, state)
            if c == 0:
                items = eng.apply_chat_prefix(items)
                for u, it in enumerate(items):
                    state[u] = dict(enc_cache=it["enc_cache"], ada_cache=it["ada_cache"], pe_index=it["pe_index"])
            pe_next, prev = pipe.push(items)
            for u in range(n):
                state[u]["pe_index"] = pe_next[u]
            record(prev)
        record(pipe.flush())
        assert k == 5
        out["group lengths"] = [kv.length for kv in kvs]
    finally:
        for kv in kvs + [base]:
            kv.free()
    assert any(key[3:4] == ("group",) for key in eng._lgraphs)
    return out


@pytest.mark.gpu
def test_tiny_engine_llm_kv_bf16(dev):
    from fo.engine import FreezeOmniEngine
    path = os.path.join(ROOT, "configs", "tiny")
    with pytest.raises(ValueError, match="llm_kv"):
        FreezeOmniEngine(path, device=dev, max_sessions=4, llm_kv="fp16")
    A = FreezeOmniEngine(path, device=dev, max_sessions=8)
    B = FreezeOmniEngine(path, device=dev, max_sessions=8, llm_kv="bf16")
    assert A.llm_kv == "fp32" and A.llm.pool.k.dtype == torch.float32
    assert B.llm_kv == "bf16" and B.llm.pool.k.dtype == torch.bfloat16
    assert B.tts.pool.k.dtype == torch.float32                     # the speech decoder's pool stays fp32
    assert A.llm.pool.n_pages == B.llm.pool.n_pages                # llm_kv_tokens keeps meaning tokens
    assert 2 * B.llm.pool.bytes_per_token == A.llm.pool.bytes_per_token
    with _rounded():
        a = _tiny_flow(A, dev)
        b = _tiny_flow(B, dev)
    _same(a, b, "tiny flow")
    assert A.llm.pool.pages_in_use() == B.llm.pool.pages_in_use()


# ------------------------------------------------------------------ no GPU
def test_bytes_per_token_follows_the_dtype():
    from fo.kv import KVPool
    fp32 = KVPool(28, 4, 128, 2, 16, "cpu")
    bf16 = KVPool(28, 4, 128, 2, 16, "cpu", dtype=torch.bfloat16)
    assert fp32.bytes_per_token == 114688 and bf16.bytes_per_token == 57344   # Qwen2-7B: the reference keeps the latter
    assert fp32.k.dtype == torch.float32 and bf16.k.dtype == bf16.v.dtype == torch.bfloat16
    assert fp32.dtype == torch.float32 and bf16.dtype == torch.bfloat16
    bf16.k[:, 0] = 1.5
    bf16.copy_page(0, 1)
    assert bool((bf16.k[:, 1] == 1.5).all())
    with pytest.raises(ValueError):
        KVPool(1, 1, 32, 2, 16, "cpu", dtype=torch.float16)


def test_cli_flag_llm_kv():
    import importlib
    inf, srv = importlib.import_module("bin.inference"), importlib.import_module("bin.server")
    base = ["--model_path", "m", "--llm_path", "l", "--input_wav", "i.wav", "--output_wav", "o.wav"]
    assert inf.get_args(base).llm_kv == "fp32"
    assert inf.get_args(base + ["--llm_kv", "bf16"]).llm_kv == "bf16"
    with pytest.raises(SystemExit):
        inf.get_args(base + ["--llm_kv", "fp16"])
    assert srv.get_parser().parse_args([]).llm_kv is None          # the config's value, else fp32
    assert srv.get_parser().parse_args(["--llm_kv", "bf16"]).llm_kv == "bf16"
    with pytest.raises(SystemExit):
        srv.get_parser().parse_args(["--llm_kv", "fp8"])
