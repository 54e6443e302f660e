"""llm_kv="e4m3" through the engines: the Qwen2 stack on an FP8 paged KV -- the staged append and
fo_attention_kv8 at the one dispatch point of DecoderStack.forward, eagerly and inside the captured graphs.

Two layers at real geometry (tests/test_real_qwen2_gpu.py's engine; only the input embeddings of
tests/golden/real_qwen2_t2.npz are read): layer 0's K / V depend on no cache, so the FP8 engine's layer-0 pool must
EQUAL fo.quant.quantize_kv_rows of the fp32 engine's; captured text steps equal eager ones; a fork copies codes AND
scales.  The mode is lossy, so against the fp32-pool engine there is a drift, recorded below and bounded at twice the
record.  The tiny config runs the whole engine (listen graph, grouped listen, text steps).

Drift record (relative L2 of the last text step's 8 hidden rows against the fp32-pool engine, first MI355X run):
    e4m3 pool 1.172e-02, bf16 pool 7.326e-04.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8 = torch.float8_e4m3fn
DRIFT_E4M3 = 1.172e-02   # the record above; the kernels are deterministic, the factor 2 covers toolchain rebuilds
TEXT_IDS = [[11, 250, 3999, 17, 90210, 5, 777, 60001], [4, 4, 1234, 151000, 9, 31, 2718, 100], [1, 2, 3, 4, 5, 6, 7, 8]]


@pytest.fixture(scope="module")
def engines(dev):
    """fp32, bf16 and e4m3 pools on one weight source, built as tests/test_kv_bf16_engine_gpu.py builds its pair."""
    from fo.llm import LLMEngine
    from fo.weights import SynthSource
    from oracle import configs
    from oracle.params import all_shapes
    cfg = configs.get("real")
    cfg["llm"]["num_hidden_layers"] = 2
    src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
    eng = {kv: LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16, kv_dtype=kv)
           for kv in ("fp32", "bf16", "e4m3")}
    C = eng["e4m3"]
    assert (C.D, C.H, C.KVH, C.hd) == (3584, 28, 4, 128) and C.kv_dtype == "e4m3"
    assert C.pool.k.dtype == FP8 and C.pool.ks.dtype == torch.float32 and C.stack.kv8 and not C.stack.attn_o
    assert C.pool.n_pages == eng["fp32"].pool.n_pages
    assert C.pool.bytes_per_token == 2 * 4 * (128 + 4) * 2
    with pytest.raises(ValueError, match="kv_dtype"):
        LLMEngine(src, cfg["llm"], dev, kv_tokens=64, page_size=16, kv_dtype="fp8")
    return eng


@pytest.fixture(scope="module")
def gold():
    from goldenio import load_golden
    return load_golden("real_qwen2_t2.npz")


def _layer0(llm, seqs):
    """Layer 0's rows of the sequences in position order, on the CPU: (K, V[, K scales, V scales])."""
    dev = llm.device
    sl = torch.tensor([q.slot(p) for q in seqs for p in range(q.length)], dtype=torch.long, device=dev)
    PS = llm.pool.PS
    pick = lambda t: t[0][sl // PS, :, sl % PS].cpu()
    k, v = llm.pool.k, llm.pool.v
    if llm.pool.fp8:
        return pick(k.view(torch.uint8)), pick(v.view(torch.uint8)), pick(llm.pool.ks), pick(llm.pool.vs)
    return pick(k), pick(v)


def _flow(llm, dev, gold):
    """The 128-row prefill (8 sessions), a 16-row chunk, an 8-row eager text step, then three steps of a captured
    TextGraph -- the same fixed ids for every engine, so layer 0's K / V are the same whatever the cache holds.  Forks
    taken before the captured steps run the same three steps eagerly.  Returns the hidden rows and layer 0's rows."""
    from fo import ops
    from fo.engine import TextGraph
    B = 8
    rows0 = gold["rows0"].tolist()
    seqs = [llm.new_seq() for _ in range(B)]
    forks = []
    out = {}
    try:
        ops.kv8_launch_counts_reset()
        for s, rows in ((0, rows0), (1, [2] * B)):
            x = torch.from_numpy(gold[f"emb{s}"].astype(np.float32)).to(dev)
            assert x.shape[0] == sum(rows) == (128 if s == 0 else 16)
            h, _ = llm.forward(x, list(zip(seqs, rows)))
            out[f"hid{s}"] = h[:sum(rows)].clone()
        x = llm.embed(TEXT_IDS[2], round_fp16=True)
        h, _ = llm.forward(x, [(q, 1) for q in seqs])
        out["hid2"] = h[:B].clone()
        if llm.pool.fp8:   # one append and one attention per layer and forward
            assert ops.kv8_launch_counts() == {"kv8_append": 6, "kv8_attention": 6}
        else:
            assert not any(ops.kv8_launch_counts().values())
        forks = [q.fork() for q in seqs]
        g = TextGraph(SimpleNamespace(device=dev, llm=llm), B, 2048, 1, 0.0, 1.0, 0)
        try:
            for j, ids in enumerate(TEXT_IDS):
                _, hid = g.run([(q, [t]) for q, t in zip(seqs, ids)])
                out[f"graph{j}"] = hid.clone()
        finally:
            g.destroy()
        for j, ids in enumerate(TEXT_IDS):
            h, _ = llm.forward(llm.embed(ids, round_fp16=True), [(q, 1) for q in forks])
            out[f"eager{j}"] = h[:B].clone()
        torch.cuda.synchronize()
        assert [q.length for q in seqs] == [q.length for q in forks] == [r + 6 for r in rows0]
        out["layer0"] = _layer0(llm, seqs)
        out["layer0_forks"] = _layer0(llm, forks)
    finally:
        for q in seqs + forks:
            q.free()
    assert llm.pool.pages_in_use() == 0
    return out


@pytest.fixture(scope="module")
def flows(dev, engines, gold):
    from fo import ops
    with torch.cuda.stream(ops.engine_stream(dev)):   # (the TextGraph's stream: a fork's page copy is ordered with it)
        return {kv: _flow(llm, dev, gold) for kv, llm in engines.items()}


def test_layer0_pool_is_the_model_of_the_fp32_pool(flows):
    """Prefill, chunk, eager and captured text steps: layer 0 of the FP8 pool == quantize_kv_rows(fp32 layer 0)."""
    from fo.quant import quantize_kv_rows
    for which in ("layer0", "layer0_forks"):
        k32, v32 = flows["fp32"][which]
        k8, v8, ks8, vs8 = flows["e4m3"][which]
        assert k32.shape[0] == 128 + 16 + 8 + 24 and k32.shape[1:] == (4, 128)
        for name, x, codes, scales in (("k", k32, k8, ks8), ("v", v32, v8, vs8)):
            q, e, _ = quantize_kv_rows(x)
            want = torch.ldexp(torch.ones_like(scales), e)
            print(f"[kv e4m3 engine] {which} {name}: {q.numel()} codes, {int((codes != q).sum())} differ; {e.numel()} "
                  f"scales, {int((scales != want).sum())} differ; exponents {sorted(set(e.flatten().tolist()))}")
            assert torch.equal(codes, q), (which, name)
            assert torch.equal(scales, want), (which, name)


def test_captured_text_steps_equal_eager_ones(flows):
    f = flows["e4m3"]
    for j in range(len(TEXT_IDS)):
        a, b = f[f"graph{j}"], f[f"eager{j}"]
        print(f"[kv e4m3 engine] text step {j}: {a.numel()} elements, {int((a != b).sum())} differ graph / eager")
        assert not torch.isnan(a).any() and torch.equal(a, b), j


def test_drift_against_the_fp32_pool(flows):
    """Relative L2 of the last text step's hidden rows against the fp32-pool engine: at most twice the recorded value,
    and strictly more than the bf16 pool's (the cache really is narrower)."""
    last = f"graph{len(TEXT_IDS) - 1}"
    ref = flows["fp32"][last].double()
    drift = {kv: float((flows[kv][last].double() - ref).norm() / ref.norm()) for kv in ("bf16", "e4m3")}
    print(f"[kv e4m3 engine] drift of the last hidden rows against the fp32 pool: e4m3 {drift['e4m3']:.3e}, "
          f"bf16 {drift['bf16']:.3e} (recorded e4m3 {DRIFT_E4M3:.3e})")
    assert drift["e4m3"] <= 2 * DRIFT_E4M3, drift
    assert drift["e4m3"] > drift["bf16"] > 0, drift


def test_copy_on_write_fork(dev, engines, gold):
    """Fork at 20 keys (a partial second page), different tokens appended to parent and child: each equals, bit for
    bit, an unforked sequence given the same appends, and the shared prefix's codes and scales are untouched."""
    llm = engines["e4m3"]
    pool = llm.pool
    emb = lambda a, b: torch.from_numpy(gold["emb0"][a:b].astype(np.float32)).to(dev)
    x0, xa, xb = emb(0, 20), emb(20, 23), emb(40, 45)
    state = lambda pages: [t[:, pages].clone() for t in (pool.k.view(torch.uint8), pool.v.view(torch.uint8), pool.ks,
                                                          pool.vs)]
    seqs = [llm.new_seq() for _ in range(3)]
    parent, ref_child, ref_parent = seqs
    try:
        hid = {}
        for name, q in (("parent", parent), ("ref_child", ref_child), ("ref_parent", ref_parent)):
            hid[name + " prompt"] = llm.forward(x0.clone(), [(q, 20)])[0][:20].clone()
        assert torch.equal(hid["parent prompt"], hid["ref_child prompt"])
        pages = torch.tensor(parent.pages, dtype=torch.long, device=dev)
        before = state(pages)
        child = parent.fork()
        seqs.append(child)
        assert child.pages == parent.pages and int(pool.ref[parent.pages[1]]) == 2
        h_child = llm.forward(xa.clone(), [(child, 3)])[0][:3].clone()
        # the child's tail page is its own copy; the parent's pages -- the shared prefix -- are untouched
        assert child.pages[0] == parent.pages[0] and child.pages[1] != parent.pages[1]
        for t, b in zip(state(pages), before):
            assert torch.equal(t, b)
        h_parent = llm.forward(xb.clone(), [(parent, 5)])[0][:5].clone()
        after = state(pages)
        for t, b in zip(after, before):   # the parent's first 20 rows: codes and scales as they were
            assert torch.equal(t[:, 0], b[:, 0]) and torch.equal(t[:, 1, :, :4], b[:, 1, :, :4])
        h_ref_child = llm.forward(xa.clone(), [(ref_child, 3)])[0][:3].clone()
        h_ref_parent = llm.forward(xb.clone(), [(ref_parent, 5)])[0][:5].clone()
        torch.cuda.synchronize()
        print(f"[kv e4m3 engine] fork: child rows differ in {int((h_child != h_ref_child).sum())}, parent rows in "
              f"{int((h_parent != h_ref_parent).sum())} elements from the unforked sequences")
        assert not torch.isnan(h_child).any() and torch.equal(h_child, h_ref_child)
        assert not torch.isnan(h_parent).any() and torch.equal(h_parent, h_ref_parent)

        def rows(q):   # every layer's codes and scales of a sequence, in position order
            sl = torch.tensor([q.slot(p) for p in range(q.length)], dtype=torch.long, device=dev)
            return [t[:, sl // pool.PS, :, sl % pool.PS] for t in (pool.k.view(torch.uint8), pool.v.view(torch.uint8),
                                                                    pool.ks, pool.vs)]

        assert [q.length for q in (parent, child, ref_parent, ref_child)] == [25, 23, 25, 23]
        for a, b in zip(rows(child) + rows(parent), rows(ref_child) + rows(ref_parent)):
            assert torch.equal(a, b)
    finally:
        for q in seqs:
            q.free()
    assert pool.pages_in_use() == 0


def test_tiny_engine_llm_kv_e4m3(dev):
    """The whole tiny engine on an FP8 pool: the captured ListenGraph, the eager listen, the grouped listen and text
    steps run on it, with the q|k|v projections under weight-only FP8 beside it, and give finite outputs."""
    from fo.engine import FreezeOmniEngine
    from test_kv_bf16_engine_gpu import _tiny_flow
    path = os.path.join(ROOT, "configs", "tiny")
    with pytest.raises(ValueError, match="llm_kv"):
        FreezeOmniEngine(path, device=dev, max_sessions=4, llm_kv="fp8")
    A = FreezeOmniEngine(path, device=dev, max_sessions=8)
    C = FreezeOmniEngine(path, device=dev, max_sessions=8, llm_kv="e4m3", attn_weights="fp8")
    assert C.llm_kv == "e4m3" and C.llm.pool.k.dtype == C.llm.pool.v.dtype == FP8
    assert C.llm.pool.ks.dtype == torch.float32 and C.llm.stack.kv8
    assert C.tts.pool.k.dtype == torch.float32 and not C.tts.main.kv8       # the speech decoder's pool stays fp32
    assert A.llm.pool.n_pages == C.llm.pool.n_pages                          # llm_kv_tokens keeps meaning tokens
    assert C.llm.pool.bytes_per_token == 2 * 2 * (32 + 4) * 2
    from fo import ops
    ops.kv8_launch_counts_reset()
    c = _tiny_flow(C, dev)
    n = ops.kv8_launch_counts()
    assert n["kv8_append"] > 0 and n["kv8_append"] == n["kv8_attention"], n
    assert len(C._lgraphs) >= 1 and len(C._tgraphs) >= 1
    for k, v in c.items():
        if torch.is_tensor(v):
            assert bool(torch.isfinite(v).all()), k
        elif k.endswith("probs"):
            assert all(np.isfinite(p) and 0.0 <= p <= 1.0 for pair in v for p in pair), (k, v)
    assert min(c["group lengths"]) > 0 and min(c["listen g1 lengths"]) > 0
