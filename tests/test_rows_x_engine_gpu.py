"""rows_x="bf16" through the engines: the Qwen2 stack's 65..128-row forwards with bf16 GEMM inputs.

Two layers at real geometry (tests/test_kv_e4m3_engine_gpu.py's engines; the inputs of tests/golden/real_qwen2_t2.npz),
one weight source, rows_x "fp32" and "bf16":
  * without a 128-row forward the two engines are the same engine: a 16-row chunk, an eager 8-row text step and three
    captured TextGraph steps give torch.equal hidden rows and pool rows, and the bf16-X counter stays 0;
  * the 128-row prefill takes the bf16 form in all four GEMMs of both layers (the counter rises by 4 x 2, gemm_rows is
    the same in both engines), and layer 0's K / V rows -- which depend on no cache -- EQUAL what the fp32 engine's
    layer-0 q|k|v writes from ops.rmsnorm(x0).bfloat16().float();
  * the drift against the fp32 engine is strictly positive and at most twice the record below;
  * against the reference-run golden (real_qwen2_group_t2.npz, the C = 8 harness of
    tests/test_real_qwen2_gpu.py::test_qwen2_real_geometry_listen_groups_match_reference, copied here: groups of 8 + 7
    chunks, captured) -- see the record below;
  * mlp_weights="mxfp4" beside it: the bf16 images forward the arm (the prefill still counts 8), the <= 16-row steps
    are bit-equal to the mxfp4 engine without the option;
  * the tiny FreezeOmniEngine (every weight under 16 MiB) with llm_rows_x="bf16" is bit for bit the default engine.

Records (first MI355X run; the kernels are deterministic, the factors 2 cover toolchain rebuilds):
    drift, relative L2 against the fp32 engine: the 128-row prefill's last hidden rows 1.087e-03, the hidden rows of
    the 16-row chunk after it 4.685e-04.
    against the reference-run golden (which the reference computed in fp32), worst deviations over the prefill and the
    15 chunks: rows_x fp32 hidden 2.110e-05, state probs 1.252e-06, row sums 4.032e-04, row sums of squares 3.491e-07
    relative; rows_x bf16 hidden 4.942e-03 (prefill last rows 4.865e-03), state probs 4.368e-04, row sums 1.905e-01,
    row sums of squares 1.397e-05 relative.  The bf16 arm MISSES the fp32-calibrated hidden bound (2e-3 abs) and meets
    the state-probability one (5e-4): its hidden rows are held to twice the record, its state probabilities to 5e-4.
    Nothing is widened for the fp32 engine.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIFT_PREFILL = 1.087e-03   # the records above
DRIFT_CHUNK = 4.685e-04
HID_RECORD = 4.942e-03      # the bf16 arm's worst hidden deviation from the reference-run golden (fp32 bound: 2e-3)
HID_BOUND, PROB_BOUND = 2 * HID_RECORD, 5e-4
TEXT_IDS = [[11, 250, 3999, 17, 90210, 5, 777, 60001], [4, 4, 1234, 151000, 9, 31, 2718, 100], [1, 2, 3, 4, 5, 6, 7, 8]]
B = 8


@pytest.fixture(scope="module")
def gold():
    from goldenio import load_golden
    return load_golden("real_qwen2_t2.npz")


def _engines(dev, **kw):
    from fo.llm import LLMEngine
    from fo.weights import SynthSource
    from oracle import configs
    from oracle.params import all_shapes
    cfg = configs.get("real")
    cfg["llm"]["num_hidden_layers"] = 2
    src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
    eng = {rx: LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16, rows_x=rx, **kw) for rx in ("fp32", "bf16")}
    for rx, e in eng.items():
        assert (e.D, e.H, e.KVH, e.hd) == (3584, 28, 4, 128) and e.rows_x == e.stack.rows_x == rx
    with pytest.raises(ValueError, match="llm_rows_x"):
        LLMEngine(src, cfg["llm"], dev, kv_tokens=64, page_size=16, rows_x="fp16")
    return eng


@pytest.fixture(scope="module")
def engines(dev):
    return _engines(dev)


def _pool_rows(llm, seqs):
    """Every layer's K and V rows of the sequences, in position order."""
    sl = torch.tensor([q.slot(p) for q in seqs for p in range(q.length)], dtype=torch.long, device=llm.device)
    PS = llm.pool.PS
    return [t[li][sl // PS, :, sl % PS].clone() for t in (llm.pool.k, llm.pool.v) for li in range(t.shape[0])]


def _small_flow(llm, dev, gold):
    """Fresh sequences, NO 128-row forward: a 16-row chunk, an eager 8-row text step, three captured TextGraph steps."""
    from fo import ops
    from fo.engine import TextGraph
    seqs = [llm.new_seq() for _ in range(B)]
    out = {}
    try:
        ops.rows_xb_launch_count_reset()
        x = torch.from_numpy(gold["emb1"].astype(np.float32)).to(dev)
        assert x.shape[0] == 16
        h, _ = llm.forward(x, [(q, 2) for q in seqs])
        out["chunk"] = h[:16].clone()
        h, _ = llm.forward(llm.embed(TEXT_IDS[2], round_fp16=True), [(q, 1) for q in seqs])
        out["eager"] = h[:B].clone()
        g = TextGraph(SimpleNamespace(device=dev, llm=llm), B, 2048, 1, 0.0, 1.0, 0)
        try:
            for j, ids in enumerate(TEXT_IDS):
                _, hid = g.run([(q, [t]) for q, t in zip(seqs, ids)])
                out[f"graph{j}"] = hid.clone()
        finally:
            g.destroy()
        torch.cuda.synchronize()
        assert [q.length for q in seqs] == [6] * B
        out["pool"] = _pool_rows(llm, seqs)
        out["xb"] = ops.rows_xb_launch_count()
    finally:
        for q in seqs:
            q.free()
    assert llm.pool.pages_in_use() == 0
    return out


def _same_small_flow(a, b, what):
    for k in a:
        if k in ("pool", "xb"):
            continue
        assert not torch.isnan(a[k]).any() and torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))
    assert len(a["pool"]) == 4
    for i, (p, q) in enumerate(zip(a["pool"], b["pool"])):
        assert p.shape == (6 * B, 4, 128) and torch.equal(p, q), (what, "pool", i)
    assert a["xb"] == b["xb"] == 0, (what, a["xb"], b["xb"])


def _prefill_flow(llm, dev, gold, scratch_from=None):
    """The 128-row prefill (8 ragged sessions) and a 16-row chunk after it.  scratch_from: an engine whose layer-0 q|k|v
    (unarmed) writes ops.rmsnorm(x0).bfloat16().float() into a scratch cache at this prefill's positions and slots."""
    from fo import ops
    rows0 = gold["rows0"].tolist()
    seqs = [llm.new_seq() for _ in range(B)]
    out = {}
    try:
        x0 = torch.from_numpy(gold["emb0"].astype(np.float32)).to(dev)
        assert x0.shape[0] == sum(rows0) == 128
        ops.launch_counts_reset()
        ops.rows_xb_launch_count_reset()
        h, bm = llm.forward(x0.clone(), list(zip(seqs, rows0)))
        torch.cuda.synchronize()
        out["counts"] = ops.launch_counts()
        out["xb"] = ops.rows_xb_launch_count()
        out["hid0"] = h[bm.last_rows_host].clone()
        sl = bm.tok_slot[:128].long()
        PS = llm.pool.PS
        out["k0"], out["v0"] = (t[0][sl // PS, :, sl % PS].clone() for t in (llm.pool.k, llm.pool.v))
        if scratch_from is not None:
            A = scratch_from
            L0 = A.stack.layers[0]
            hn = ops.rmsnorm(x0, L0.ln1, A.eps, out=torch.empty_like(x0), round_fp16=A.stack.first_fp16)
            hr = hn.bfloat16().float()
            assert not torch.equal(hn, hr)
            kc, vc = (torch.full_like(t[0], -768.0) for t in (llm.pool.k, llm.pool.v))
            q = torch.empty(128, A.H * A.hd, device=dev)
            n = ops.rows_xb_launch_count()
            L0.qkv.qkv_rope(hr, 128, bm.tok_pos, bm.tok_slot, A.rope[0], A.rope[1], q, kc, vc, A.H, A.KVH, PS)
            assert ops.rows_xb_launch_count() == n   # (unarmed: the fp32 arm on bf16-valued rows)
            out["k0_model"], out["v0_model"] = kc[sl // PS, :, sl % PS].clone(), vc[sl // PS, :, sl % PS].clone()
        x1 = torch.from_numpy(gold["emb1"].astype(np.float32)).to(dev)
        n = ops.rows_xb_launch_count()
        h, _ = llm.forward(x1, [(q_, 2) for q_ in seqs])
        out["hid1"] = h[:16].clone()
        torch.cuda.synchronize()
        assert ops.rows_xb_launch_count() == n    # the 16-row chunk takes no bf16 form
    finally:
        for q_ in seqs:
            q_.free()
    assert llm.pool.pages_in_use() == 0
    return out


@pytest.fixture(scope="module")
def prefills(dev, engines, gold):
    from fo import ops
    with torch.cuda.stream(ops.engine_stream(dev)):
        a = _prefill_flow(engines["fp32"], dev, gold)
        b = _prefill_flow(engines["bf16"], dev, gold, scratch_from=engines["fp32"])
    return {"fp32": a, "bf16": b}


def test_without_a_128_row_forward_the_engines_are_the_same(dev, engines, gold):
    from fo import ops
    with torch.cuda.stream(ops.engine_stream(dev)):
        a, b = (_small_flow(engines[rx], dev, gold) for rx in ("fp32", "bf16"))
    _same_small_flow(a, b, "rows_x bf16 vs fp32")


def test_prefill_takes_the_bf16_form_in_every_gemm(prefills):
    a, b = prefills["fp32"], prefills["bf16"]
    nl = 2
    assert a["xb"] == 0 and b["xb"] == 4 * nl, (a["xb"], b["xb"])
    assert a["counts"]["gemm_rows"] == b["counts"]["gemm_rows"] == 4 * nl, (a["counts"], b["counts"])
    assert a["counts"] == b["counts"]
    # layer 0 depends on no cache: its K / V are the fp32 arm's on the bf16-rounded normed rows, bit for bit
    for n in ("k0", "v0"):
        got, want = b[n], b[n + "_model"]
        print(f"[rows x engine] layer 0 {n}: {got.numel()} elements, {int((got != want).sum())} differ from the model, "
              f"{int((got != a[n]).sum())} from the fp32 engine")
        assert got.shape == (128, 4, 128) and not torch.isnan(got).any()
        assert torch.equal(got, want), n
        assert not torch.equal(got, a[n]), n


def test_drift_against_the_fp32_engine(prefills):
    a, b = prefills["fp32"], prefills["bf16"]
    rel = lambda k: float((b[k].double() - a[k].double()).norm() / a[k].double().norm())
    d0, d1 = rel("hid0"), rel("hid1")
    print(f"[rows x engine] drift against the fp32 engine (relative L2): prefill last rows {d0:.3e} (record "
          f"{DRIFT_PREFILL:.3e}), next 16-row chunk {d1:.3e} (record {DRIFT_CHUNK:.3e})")
    assert 0 < d0 <= 2 * DRIFT_PREFILL, d0
    assert 0 < d1 <= 2 * DRIFT_CHUNK, d1


# ------------------------------------------------------------------ against the reference-run golden
def _group_embeds(chunk, b, D=3584):
    """tests/golden/make_golden.py group_embeds: the fp16-valued inputs of the listen chunks (regenerated, checksummed)."""
    return (np.random.default_rng(8765 + 100 * chunk + b).standard_normal((2, D)) * 0.5).astype(np.float16)


def _listen_groups(llm, dev, gold, grp, C=8):
    """The C = 8 harness of tests/test_real_qwen2_gpu.py's listen-groups test (groups of 8 + 7 chunks, each distinct m
    captured on the engine stream and replayed) on `llm`; returns the worst deviations from the golden and the bf16-X
    counter's rise at each capture instead of asserting the tolerances."""
    from fo import _lib, ops
    from fo.engine import ListenGraph, _HostRing
    from fo.kv import GroupMeta
    lib = _lib.load()
    assert lib.fo_gemm_set_pipe(3) >= -1
    To, D = 2, llm.D
    NC = int(grp["n_chunks"])
    n1, nl = B * To, len(llm.stack.layers)
    cols = grp["cols"]
    rows0 = gold["rows0"].tolist()
    seqs = [llm.new_seq() for _ in range(B)]
    main = ops.engine_stream(dev)
    execs, ring = {}, None
    insum = 0.0
    dev_ = {"prefill": 0.0, "hidden": 0.0, "probs": 0.0, "hsum": 0.0, "hsq_rel": 0.0, "xb": []}
    try:
        x0 = torch.from_numpy(gold["emb0"].astype(np.float32)).to(dev)
        h, bm = llm.forward(x0, [(q, r) for q, r in zip(seqs, rows0)])
        dev_["prefill"] = float(np.abs(h[bm.last_rows_host].cpu().numpy() - gold["hid0"]).max())
        torch.cuda.synchronize()
        max_keys = max(max(q.length for q in seqs) + 64 * 2 * C + 1024, 2048)
        gm = GroupMeta(B, To, C, llm.H // llm.KVH, max_keys, llm.pool.PS, dev)
        x = torch.empty(C * n1, D, dtype=torch.float32, device=dev)
        ws = llm.stack.workspace(C * n1, ops.attn_nsplit(max_keys, C * B, llm.KVH), dev)
        probs = torch.empty(C * B, 3, dtype=torch.float32, device=dev)
        ring = _HostRing(gm.size)
        with torch.cuda.stream(main):
            ops.Runtime.get(dev)

        def body(m):   # ListenGraph._llm_body
            xm = x[:m * n1]
            llm.stack.forward(xm, gm.metas[m], ws)
            ops.rmsnorm(xm, llm.norm, llm.eps, out=xm)
            ops.state_head(xm, gm.rows[:m * B], llm.head_w, llm.head_b, probs)

        for c0 in range(0, NC, C):
            m = min(C, NC - c0)
            M = m * n1
            what = f"chunks {c0}..{c0 + m - 1} (M = {M})"
            if m not in execs:
                ops.launch_counts_reset()
                ops.rows_xb_launch_count_reset()
                execs[m] = ListenGraph._capture(main, lambda: body(m))
                c = ops.launch_counts()
                assert M > 64 and c["gemm_rows"] == 4 * nl and c["gemm_xsk"] == 0, (what, c)
                assert c["attn_mfma"] == nl and c["attn_decode"] == 0, (what, c)
                dev_["xb"].append(ops.rows_xb_launch_count())
            xs = np.empty((M, D), np.float16)
            for j in range(m):
                for b in range(B):
                    e = _group_embeds(c0 + j, b)
                    insum += float(e.astype(np.float64).sum())
                    xs[j * n1 + b * To:j * n1 + (b + 1) * To] = e
            k, hb = ring.next()
            gm.fill(hb, seqs, m)
            with torch.cuda.stream(main):
                x[:M].copy_(torch.from_numpy(xs.astype(np.float32)), non_blocking=False)
            ring.upload(k, gm.buf, main)
            _lib.call("fo_graph_launch", execs[m], main.cuda_stream)
            main.synchronize()
            assert [q.length for q in seqs] == grp["kvlen"][c0 + m - 1].tolist(), what
            hv = x[:M].cpu().numpy().reshape(m, B, To, D)
            assert np.isfinite(hv).all()
            h64 = hv.astype(np.float64)
            want = slice(c0, c0 + m)
            dev_["hidden"] = max(dev_["hidden"], float(np.abs(hv[:, :, -1] - grp["hlast"][want]).max()),
                                 float(np.abs(hv[..., cols] - grp["hcols"][want]).max()))
            dev_["hsum"] = max(dev_["hsum"], float(np.abs(h64.sum(-1) - grp["hsum"][want]).max()))
            dev_["hsq_rel"] = max(dev_["hsq_rel"], float(np.abs((h64 ** 2).sum(-1) / grp["hsq"][want] - 1).max()))
            p = probs[:m * B].cpu().numpy().reshape(m, B, 3)
            dev_["probs"] = max(dev_["probs"], float(np.abs(p - grp["probs"][want]).max()))
        assert sorted(execs) == [7, 8]
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
    return dev_


def test_listen_groups_against_the_reference(dev, engines, gold):
    from goldenio import load_golden
    grp = load_golden("real_qwen2_group_t2.npz")
    d = {rx: _listen_groups(engines[rx], dev, gold, grp) for rx in ("fp32", "bf16")}
    for rx, v in d.items():
        print(f"[rows x engine] rows_x {rx} against the reference-run golden: worst hidden deviation {v['hidden']:.3e}, "
              f"state probs {v['probs']:.3e}, prefill last rows {v['prefill']:.3e}, row sums {v['hsum']:.3e}, row sums of "
              f"squares {v['hsq_rel']:.3e} relative; bf16-X launches per capture {v['xb']}")
    a, b = d["fp32"], d["bf16"]
    assert a["xb"] == [0, 0] and b["xb"] == [4 * 2, 4 * 2]
    # the fp32 engine: the bounds of the listen-groups test, unchanged
    assert a["prefill"] <= 2e-3 and a["hidden"] <= 2e-3 and a["probs"] <= 5e-4, a
    assert a["hsum"] <= 2e-3 * 3584 ** 0.5 and a["hsq_rel"] <= 1e-4, a
    # the bf16 arm: hidden rows at twice the record (the mode misses 2e-3), state probabilities at the fp32 bound
    assert b["hidden"] > 2e-3   # (should this ever fail, the mode meets the fp32 bound: assert that one instead)
    assert b["prefill"] <= HID_BOUND and b["hidden"] <= HID_BOUND and b["probs"] <= PROB_BOUND, b


# ------------------------------------------------------------------ one combination, and the tiny engine
def test_mxfp4_mlp_beside_it(dev, gold):
    """mlp_weights="mxfp4" with rows_x="bf16": at 128 rows the quantised layers run their bf16 images, which forward
    the arm; the <= 16-row steps (streamed codes, fp32 rows) are bit-equal to the mxfp4 engine without the option."""
    from fo import ops
    eng = _engines(dev, mlp_weights="mxfp4")
    with torch.cuda.stream(ops.engine_stream(dev)):
        a, b = (_small_flow(eng[rx], dev, gold) for rx in ("fp32", "bf16"))
        _same_small_flow(a, b, "mxfp4, rows_x bf16 vs fp32")
        pa, pb = (_prefill_flow(eng[rx], dev, gold) for rx in ("fp32", "bf16"))
    assert pa["xb"] == 0 and pb["xb"] == 4 * 2, (pa["xb"], pb["xb"])
    assert pa["counts"] == pb["counts"] and pb["counts"]["gemm_rows"] == 4 * 2, pb["counts"]
    assert not torch.equal(pa["hid0"], pb["hid0"]) and bool(torch.isfinite(pb["hid0"]).all())


def test_tiny_engine_llm_rows_x_bf16(dev):
    """Every weight of the tiny config is under 16 MiB: no launch takes the bf16 form, and the grouped listen, the
    captured and eager listens and the text steps are bit for bit the default engine's."""
    from fo import ops
    from fo.engine import FreezeOmniEngine
    from test_kv_bf16_engine_gpu import _tiny_flow
    path = os.path.join(ROOT, "configs", "tiny")
    with pytest.raises(ValueError, match="llm_rows_x"):
        FreezeOmniEngine(path, device=dev, max_sessions=4, llm_rows_x="fp16")
    A = FreezeOmniEngine(path, device=dev, max_sessions=8)
    C = FreezeOmniEngine(path, device=dev, max_sessions=8, llm_rows_x="bf16")
    assert A.llm_rows_x == "fp32" and C.llm_rows_x == C.llm.rows_x == C.llm.stack.rows_x == "bf16"
    assert C.tts.main.rows_x == "fp32"   # the speech decoder's stack is untouched
    ops.rows_xb_launch_count_reset()
    a, c = _tiny_flow(A, dev), _tiny_flow(C, dev)
    assert ops.rows_xb_launch_count() == 0
    assert a.keys() == c.keys()
    for k, v in a.items():
        if torch.is_tensor(v):
            assert bool(torch.isfinite(v).all()) and torch.equal(v, c[k]), k
        else:
            assert v == c[k], k
