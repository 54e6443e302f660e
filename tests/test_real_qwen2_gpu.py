"""Qwen2-7B at REAL geometry on the HIP path against the REFERENCE ITSELF (tests/golden/real_qwen2_t2.npz,
made by tests/golden/make_golden.py real_qwen2 through the reference's AudioLLM._llm_forward_core /
_prediction_head_forward / _post_decode on a 2-layer Qwen2ForCausalLM at hidden 3584, 28 q / 4 kv heads of
128, intermediate 18944, rope_theta 1e6, vocab 152,064; models/audioLLM.py:70-74,431-477,479-493).

Eight ragged sessions batched the way the engine batches them: one prefill of 9..23 rows each (M = 128,
the many-row-tile GEMMs), two listen-shaped chunks of 2 rows each (M = 16: the X-stationary k_gemm_xs
gate/up, the pipelined k_gemm_wpipe down + reduce, k_attn_mfma<128> with the 7:1 GQA grouping, RoPE at
head_dim 128), then three text steps of 1 row each replayed from a captured TextGraph (M = 8: embedding
rows rounded to fp16, the layers, final norm, the 152,064-row lm_head, the top_k = 1 sampler).
The reference computes in fp32 with the same bf16-valued weights; the HIP path uses bf16 weights with fp32
activations (bf16 hi/lo split).  Tolerances (written here): hidden rows 2e-3 abs, state probs 5e-4,
logits 1e-3 abs + 1e-3 rel (north_star), greedy ids exact (every reference top-2 margin here is >= 5.6e-3),
_post_decode's pre-multinomial probs at V = 152,064: kept set exact, values 1e-6 abs / 1e-4 rel.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from goldenio import load_golden
from oracle import configs
from oracle.params import all_shapes

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return load_golden("real_qwen2_t2.npz")


@pytest.fixture(scope="module")
def llm(dev):
    from fo.llm import LLMEngine
    from fo.weights import SynthSource
    cfg = configs.get("real")
    cfg["llm"]["num_hidden_layers"] = 2
    src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
    eng = LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16)
    assert (eng.D, eng.H, eng.KVH, eng.V) == (3584, 28, 4, 152064)
    return eng


def _close(a, b, atol, rtol=0.0, what=""):
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    np.testing.assert_allclose(a, b, atol=atol, rtol=rtol, err_msg=what)


def _check_logits(lg, gold, first, what):
    """lg: device [B, V] logits of decision rows first..first+B-1 (dec_* order: session-major, 4 per session)."""
    lg = lg.float().cpu().numpy()
    fixed = gold["fixed_idx"]
    for b in range(lg.shape[0]):
        r = first + 4 * b
        row = lg[b]
        assert int(row.argmax()) == int(gold["dec_argmax"][r]), (what, b, int(row.argmax()), int(gold["dec_argmax"][r]))
        _close(row[gold["dec_top_ids"][r]], gold["dec_top_vals"][r], 1e-3, 1e-3, f"{what} top-32 b{b}")
        _close(row[fixed], gold["dec_fixed"][r], 1e-3, 1e-3, f"{what} fixed-index b{b}")
        lse = float(np.logaddexp.reduce(row.astype(np.float64)))
        assert abs(lse - float(gold["dec_lse"][r])) < 1e-3, (what, b, lse, float(gold["dec_lse"][r]))


def test_qwen2_real_geometry_matches_reference(dev, llm, gold):
    check_llm_against_golden(llm, dev, gold)


def check_llm_against_golden(llm, dev, gold):
    """The golden's prefill, two chunks and three text steps through `llm` (an LLMEngine at the golden's
    geometry: synthetic weights here, the reference's file formats in test_real_ingestion_gpu.py)."""
    from fo import _lib, ops
    from fo.engine import TextGraph
    lib = _lib.load()
    assert lib.fo_gemm_set_pipe(3) >= -1   # the default policy (what the bench runs)
    B = 8
    rows0 = gold["rows0"].tolist()
    assert sum(rows0) == 128
    seqs = [llm.new_seq() for _ in range(B)]
    probs_want = gold["probs"]
    try:
        # steps 0-2: prefill (M = 128), two 2-row chunks (M = 16)
        for s, rows in ((0, rows0), (1, [2] * B), (2, [2] * B)):
            x = torch.from_numpy(gold[f"emb{s}"].astype(np.float32)).to(dev)
            h, bm = llm.forward(x, [(q, r) for q, r in zip(seqs, rows)])
            last = bm.last_rows_host
            if s == 0:
                _close(h[last], gold["hid0"], 2e-3, 0, "prefill last rows")
            else:
                _close(h[:sum(rows)], gold[f"hid{s}"], 2e-3, 0, f"chunk {s} rows")
            p = llm.state_probs(h, last).cpu().numpy()
            _close(p, probs_want[s], 5e-4, 0, f"state probs step {s}")
        assert [q.length for q in seqs] == [r + 4 for r in rows0]
        # decision row of the last chunk: lm_head (M = 8) and the greedy pick
        lg = llm.logits(h, last)
        _check_logits(lg, gold, 0, "chunk-2 logits")
        _close(lg[0], gold["full_b0_s2"], 1e-3, 1e-3, "full logits row b0/s2")
        ids = torch.empty(B, dtype=torch.int32, device=dev)
        ops.sample(lg, llm.V, ids, torch.ones(B, dtype=torch.int32, device=dev))
        assert ids.cpu().tolist() == gold["toks"][0].tolist()
        # steps 3-5: text steps from a captured TextGraph (the engine's decode path), fed the reference's tokens
        g = TextGraph(SimpleNamespace(device=dev, llm=llm), B, 2048, 1, 0.0, 1.0, 0)
        try:
            for s in (3, 4, 5):
                feed = gold["toks"][s - 3].tolist()
                got, hid = g.run([(q, [t]) for q, t in zip(seqs, feed)])
                _close(hid, gold[f"hid{s}"], 2e-3, 0, f"text step {s} hidden")
                p = llm.state_probs(hid, list(range(B))).cpu().numpy()
                _close(p, probs_want[s], 5e-4, 0, f"state probs step {s}")
                _check_logits(g.logits, gold, s - 2, f"text step {s} logits")
                if s == 3:
                    _close(g.logits[1], gold["full_b1_s3"], 1e-3, 1e-3, "full logits row b1/s3")
                assert got == gold["toks"][s - 2].tolist(), (s, got, gold["toks"][s - 2].tolist())
        finally:
            g.destroy()
        assert [q.length for q in seqs] == [r + 7 for r in rows0]
    finally:
        for q in seqs:
            q.free()
    assert llm.pool.pages_in_use() == 0


def test_post_decode_probs_at_full_vocabulary_match_reference(dev, gold):
    """fo_sample_probs on the reference's own 152,064-wide logits rows against _post_decode's
    pre-multinomial probs: top_k in {0 (full vocabulary, radix select), 1, 20 (block arg-max), 100 (radix)}
    x top_p in {0, 0.8}."""
    from fo import ops
    rows = np.stack([gold["full_b0_s2"], gold["full_b1_s3"]])
    B, V = rows.shape
    lg = torch.from_numpy(rows).to(dev)
    want_all = gold["sampler_probs"]
    for si, (T, k, p) in enumerate(gold["sampler_settings"]):
        probs = torch.empty(B, V, dtype=torch.float32, device=dev)
        ids = torch.empty(B, dtype=torch.int32, device=dev)
        ops.sample_probs(lg, V, ids, probs, torch.full((B,), int(k), dtype=torch.int32, device=dev),
                         torch.full((B,), float(T), device=dev), torch.full((B,), float(p), device=dev), seed=11,
                         step=torch.arange(B, dtype=torch.int32, device=dev))
        got = probs.cpu().numpy()
        want = want_all[:, si]
        np.testing.assert_array_equal(got > 0, want > 0, err_msg=f"kept set, setting {(T, k, p)}")
        np.testing.assert_allclose(got, want, atol=1e-6, rtol=1e-4, err_msg=f"setting {(T, k, p)}")
        drawn = ids.cpu().numpy()
        assert all(want[b, drawn[b]] > 0 for b in range(B)), (si, drawn)


# ------------------------------------------------------------------ 17..64-row steps (duplex ticks, assistant prefix)
def _mid_embeds(step, b, rows, D=3584):
    """tests/golden/make_golden.py mid_embeds: the fp16-valued inputs of the mid steps (regenerated, checksummed)."""
    return (np.random.default_rng(4321 + 100 * step + b).standard_normal((rows, D)) * 0.5).astype(np.float16)


def test_qwen2_real_geometry_17_to_64_row_steps_match_reference(dev, llm, gold):
    """real_qwen2_mid_t2.npz (make_golden.py real_qwen2_mid: the reference's _llm_forward_core /
    _prediction_head_forward on the same 2-layer counter-hash Qwen2, each session its own DynamicCache): after the
    128-row prefill, steps of 4, 5, ragged 4..9, 6 and 8 rows per session -- M = 32, 40, 44, 48, 64 batched, the
    shapes of every duplex tick and assistant prefix -- on the DEFAULT policy: the X-stationary split-K gate/up and
    down (k_gemm_xsk + k_gemm_reduce) at 2, 3 and 4 row blocks, the mid-row RoPE q|k|v in 4-tile groups, the packed
    q|k|v / o inputs (k_gemm_xp) written by the reduce, the statistics epilogue and the attention.  The launch
    counters assert each family ran on every step, so a policy change cannot route around what this test pins.
    Tolerances as the other real-geometry steps: hidden 2e-3 abs (1024 fixed columns of every row, each session's
    whole last row, and each row's sum / sum of squares over all 3584 columns at 2e-3 x sqrt(3584) / relative
    1e-4), state probs 5e-4, logits 1e-3 abs + 1e-3 rel; greedy ids equal where the reference's top-2 margin
    exceeds 2e-3 (otherwise within its top 2)."""
    from fo import _lib, ops
    mid = load_golden("real_qwen2_mid_t2.npz")
    lib = _lib.load()
    assert lib.fo_gemm_set_pipe(3) >= -1
    B, D = 8, llm.D
    cols = mid["cols"]
    rows0 = gold["rows0"].tolist()
    seqs = [llm.new_seq() for _ in range(B)]
    insum = 0.0
    try:
        x = torch.from_numpy(gold["emb0"].astype(np.float32)).to(dev)
        h, bm = llm.forward(x, [(q, r) for q, r in zip(seqs, rows0)])
        _close(h[bm.last_rows_host], gold["hid0"], 2e-3, 0, "prefill last rows")
        for s in range(int(mid["n_steps"])):
            rows = mid[f"rows{s}"].tolist()
            M = sum(rows)
            xs = [_mid_embeds(s, b, rows[b]) for b in range(B)]
            insum += sum(float(v.astype(np.float64).sum()) for v in xs)
            x = torch.from_numpy(np.concatenate(xs).astype(np.float32)).to(dev)
            ops.launch_counts_reset()
            h, bm = llm.forward(x, [(q, r) for q, r in zip(seqs, rows)])
            torch.cuda.synchronize()
            c = ops.launch_counts()
            nl = len(llm.stack.layers)
            what = f"step {s} (M = {M})"
            assert c["gemm_xsk"] == 2 * nl, (what, c)          # gate/up + down per layer on the split-K stream
            assert c["gemm_rope4"] == nl, (what, c)            # q|k|v in 4-tile groups, epilogue in the reduce
            assert c["gemm_xp"] >= 2 * nl - 1, (what, c)       # o of every layer + q|k|v of layers > 0 read packed X
            assert c["attn_mfma"] == nl and c["attn_opack"] == nl, (what, c)
            assert c["gemm_ypack"] >= 2 * nl - 1, (what, c)    # o / down producers pack the next input
            hv = h[:M].float().cpu().numpy()
            _close(hv[:, cols], mid[f"hcols{s}"], 2e-3, 0, f"{what} hidden at fixed columns")
            _close(hv[bm.last_rows_host], mid[f"hlast{s}"], 2e-3, 0, f"{what} last rows")
            h64 = hv.astype(np.float64)
            np.testing.assert_allclose(h64.sum(1), mid[f"hsum{s}"], atol=2e-3 * 3584 ** 0.5, err_msg=f"{what} row sums")
            np.testing.assert_allclose((h64 ** 2).sum(1), mid[f"hsq{s}"], rtol=1e-4, err_msg=f"{what} row sumsq")
            p = llm.state_probs(h, bm.last_rows_host).cpu().numpy()
            _close(p, mid[f"probs{s}"], 5e-4, 0, f"{what} state probs")
            lg = llm.logits(h, bm.last_rows_host).float().cpu().numpy()
            for b in range(B):
                row = lg[b]
                top = mid[f"top_ids{s}"][b]
                if mid[f"margin{s}"][b] > 2e-3:
                    assert int(row.argmax()) == int(mid[f"argmax{s}"][b]), (what, b)
                else:
                    assert int(row.argmax()) in top[:2].tolist(), (what, b)
                _close(row[top], mid[f"top_vals{s}"][b], 1e-3, 1e-3, f"{what} top-32 b{b}")
                _close(row[gold["fixed_idx"]], mid[f"fixed{s}"][b], 1e-3, 1e-3, f"{what} fixed-index b{b}")
                lse = float(np.logaddexp.reduce(row.astype(np.float64)))
                assert abs(lse - float(mid[f"lse{s}"][b])) < 1e-3, (what, b, lse)
        assert abs(insum - float(mid["input_sum"])) < 1e-6 * max(1.0, abs(insum)), (insum, float(mid["input_sum"]))
    finally:
        for q in seqs:
            q.free()
    assert llm.pool.pages_in_use() == 0


# ------------------------------------------------------------------ listen groups (C chunks per Qwen2 stage)
def _group_embeds(chunk, b, D=3584):
    """tests/golden/make_golden.py group_embeds: the fp16-valued inputs of the listen chunks (regenerated, checksummed)."""
    return (np.random.default_rng(8765 + 100 * chunk + b).standard_normal((2, D)) * 0.5).astype(np.float16)


@pytest.mark.parametrize("C", [8, 4, 1])
def test_qwen2_real_geometry_listen_groups_match_reference(dev, llm, gold, C):
    """real_qwen2_group_t2.npz (make_golden.py real_qwen2_group: 15 consecutive 2-row chunks per session fed one call
    at a time to the reference's _llm_forward_core / _prediction_head_forward after the 9 + 2b-row prefill, each
    session its own DynamicCache) against the Qwen2 stage of engine.ListenGraph(chunks=C) at C chunks per stage, driven
    through the product's own tables (kv.GroupMeta: chunk-major rows, (chunk, session) items, decision rows, the
    tok_pos / tok_slot / tok_nvis / block-table fill), workspace and split count sized as _listen_graph_for sizes
    them, every distinct m captured with ListenGraph._capture on the engine stream and replayed.
      C = 8: groups of 8 + 7 chunks, M = 128 and 112 -- the benchmark's listen: the 65..128-row k_gemm_rows family on
             all four GEMMs of a layer, 64 / 56 attention items whose later chunks read the keys the earlier ones
             append in the same forward, 64 / 56 state-head rows;
      C = 4: 4 + 4 + 4 + 3, M = 64 and 48 -- the split-K 17..64-row family;
      C = 1: fifteen single chunks -- the control: golden and harness agree where nothing is grouped.
    The odd prefill lengths put a chunk across a 16-token KV page at a different chunk in each session.  The launch
    counters (read around each capture: a captured graph counts at capture) pin the kernel families, so a policy
    change cannot route around this test.  Tolerances as the other real-geometry steps: hidden 2e-3 abs (each
    chunk's whole last row, both rows at 1024 fixed columns, both rows' sum / sum of squares over all 3584 columns at
    2e-3 x sqrt(3584) / relative 1e-4), state probs 5e-4 for every chunk of every session, KV lengths exact after
    every group, the regenerated inputs' checksum to 1e-6 relative."""
    from fo import _lib, ops
    from fo.engine import ListenGraph, _HostRing
    from fo.kv import GroupMeta
    grp = load_golden("real_qwen2_group_t2.npz")
    lib = _lib.load()
    assert lib.fo_gemm_set_pipe(3) >= -1   # the default policy (what the bench runs)
    B, To, D = 8, 2, llm.D
    NC = int(grp["n_chunks"])
    assert NC == 15
    n1, nl = B * To, len(llm.stack.layers)
    cols = grp["cols"]
    rows0 = gold["rows0"].tolist()
    seqs = [llm.new_seq() for _ in range(B)]
    main = ops.engine_stream(dev)
    execs, ring = {}, None
    insum, worst = 0.0, {}   # m: [hidden, state prob] worst deviations
    try:
        x0 = torch.from_numpy(gold["emb0"].astype(np.float32)).to(dev)
        h, bm = llm.forward(x0, [(q, r) for q, r in zip(seqs, rows0)])
        _close(h[bm.last_rows_host], gold["hid0"], 2e-3, 0, "prefill last rows")
        torch.cuda.synchronize()
        # EngineCore._listen_graph_for as ListenPipe.push calls it (extra = 64 * 2 * C), ListenGraph.__init__
        max_keys = max(max(q.length for q in seqs) + 64 * 2 * C + 1024, 2048)
        gm = GroupMeta(B, To, C, llm.H // llm.KVH, max_keys, llm.pool.PS, dev)
        x = torch.empty(C * n1, D, dtype=torch.float32, device=dev)
        ws = llm.stack.workspace(C * n1, ops.attn_nsplit(max_keys, C * B, llm.KVH), dev)
        probs = torch.empty(C * B, 3, dtype=torch.float32, device=dev)
        ring = _HostRing(gm.size)
        with torch.cuda.stream(main):
            ops.Runtime.get(dev)   # the engine stream's GEMM scratch exists before anything is captured on it

        def body(m):   # ListenGraph._llm_body
            xm = x[:m * n1]
            llm.stack.forward(xm, gm.metas[m], ws)
            ops.rmsnorm(xm, llm.norm, llm.eps, out=xm)
            ops.state_head(xm, gm.rows[:m * B], llm.head_w, llm.head_b, probs)

        for c0 in range(0, NC, C):
            m = min(C, NC - c0)
            M = m * n1
            what = f"C = {C}, chunks {c0}..{c0 + m - 1} (M = {M})"
            if m not in execs:
                ops.launch_counts_reset()
                execs[m] = ListenGraph._capture(main, lambda: body(m))
                c = ops.launch_counts()
                print(f"[listen groups] {what} launches { {k: v for k, v in c.items() if v} }")
                assert c["attn_mfma"] == nl and c["attn_decode"] == 0, (what, c)
                if M > 64:    # 65..128 rows: q|k|v, o, gate/up and down (each >= 16 MiB of weights) on k_gemm_rows
                    assert c["gemm_rows"] == 4 * nl and c["gemm_xsk"] == 0, (what, c)
                elif M > 16:  # 17..64 rows: the split-K family, as the 17..64-row test above pins it
                    assert c["gemm_xsk"] == 2 * nl and c["gemm_rope4"] == nl and c["gemm_rows"] == 0, (what, c)
                    assert c["gemm_xp"] >= 2 * nl - 1 and c["gemm_ypack"] >= 2 * nl - 1, (what, c)
                    assert c["attn_opack"] == nl, (what, c)
                else:         # one chunk: neither of the many-row families
                    assert c["gemm_rows"] == 0 and c["gemm_xsk"] == 0, (what, c)
            xs = np.empty((M, D), np.float16)
            for j in range(m):
                for b in range(B):
                    e = _group_embeds(c0 + j, b)
                    insum += float(e.astype(np.float64).sum())
                    xs[j * n1 + b * To:j * n1 + (b + 1) * To] = e   # chunk-major: [chunk][session][token]
            k, hb = ring.next()
            gm.fill(hb, seqs, m)
            with torch.cuda.stream(main):
                x[:M].copy_(torch.from_numpy(xs.astype(np.float32)), non_blocking=False)
            ring.upload(k, gm.buf, main)
            _lib.call("fo_graph_launch", execs[m], main.cuda_stream)
            main.synchronize()
            assert [q.length for q in seqs] == grp["kvlen"][c0 + m - 1].tolist(), what
            hv = x[:M].cpu().numpy().reshape(m, B, To, D)
            h64 = hv.astype(np.float64)
            want = slice(c0, c0 + m)
            w = worst.setdefault(m, [0.0, 0.0])
            w[0] = max(w[0], float(np.abs(hv[:, :, -1] - grp["hlast"][want]).max()),
                       float(np.abs(hv[..., cols] - grp["hcols"][want]).max()))
            _close(hv[:, :, -1], grp["hlast"][want], 2e-3, 0, f"{what} last rows")
            _close(hv[..., cols], grp["hcols"][want], 2e-3, 0, f"{what} hidden at fixed columns")
            np.testing.assert_allclose(h64.sum(-1), grp["hsum"][want], atol=2e-3 * 3584 ** 0.5, err_msg=f"{what} row sums")
            np.testing.assert_allclose((h64 ** 2).sum(-1), grp["hsq"][want], rtol=1e-4, err_msg=f"{what} row sumsq")
            p = probs[:m * B].cpu().numpy().reshape(m, B, 3)
            w[1] = max(w[1], float(np.abs(p - grp["probs"][want]).max()))
            _close(p, grp["probs"][want], 5e-4, 0, f"{what} state probs")
        for m, w in worst.items():
            print(f"[listen groups] C = {C}, groups of {m}: worst hidden deviation {w[0]:.2e}, state probs {w[1]:.2e}")
        assert sorted(execs) == sorted({min(C, NC - c0) for c0 in range(0, NC, C)})
        assert abs(insum - float(grp["input_sum"])) < 1e-6 * max(1.0, abs(insum)), (insum, float(grp["input_sum"]))
        assert [q.length for q in seqs] == [r + 2 * NC for r in rows0]
    finally:
        torch.cuda.synchronize()
        for ex in execs.values():
            _lib.call("fo_graph_destroy", ex)
        if ring is not None:
            ring.destroy()
        for q in seqs:
            q.free()
    assert llm.pool.pages_in_use() == 0
