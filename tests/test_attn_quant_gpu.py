"""attn_weights="fp8" / "mxfp4" through the engines: the option is a MODEL (self_attn.{q,k,v,o}_proj.weight of every Qwen2
layer become q * 2^e, served dequantised by engine.src; the biases, the MLP, the head and the embedding are untouched),
not a per-launch approximation.  A bf16 engine built on the quantised engine's src holds the same packed images and
computes the same rows to the accumulation-order difference between kernels; forwards above 16 rows are bit-identical;
and the numpy oracle on the same model holds two layers at real geometry to tests/test_full_depth_gpu.py's bounds."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "configs", "tiny")
FMTS = ("fp8", "mxfp4")
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj")


def _counts():
    """(quantised q|k|v launches, fo_gemm_w8 general-form launches, fo_gemm_w4 general-form launches)."""
    from fo import ops
    return (sum(ops.qkv_quant_launch_counts().values()), ops.launch_counts()["gemm_w8"], ops.w4_launch_counts()["w4"])


def _predicted(fmt, layers, qkv=None, o=None):
    """The counters' rise over one <= 16-row forward of `layers` layers (bf16 MLP): ops.ATTN_POLICY's, or the forced
    dispatch."""
    from fo import ops
    qkv = ops.ATTN_POLICY[fmt]["qkv"] if qkv is None else qkv
    o = ops.ATTN_POLICY[fmt]["o"] if o is None else o
    return (layers * int(qkv), layers * int(o) if fmt == "fp8" else 0, layers * int(o) if fmt == "mxfp4" else 0)


def _close(a, b, what):
    a, b = (t.detach().float().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (a, b))
    np.testing.assert_allclose(a, b, atol=1e-3, rtol=1e-3, err_msg=what)


def _quantised(raw, fmt):
    from fo.quant import quantize_blocks_e2m1, quantize_rows_e4m3
    return (quantize_rows_e4m3 if fmt == "fp8" else quantize_blocks_e2m1)(raw)[2]


def _force(llm, on):
    """Every layer's q|k|v and o forced onto (True) or off (False) the code streams; returns the previous settings."""
    prev = [(L.qkv.stream, L.o.stream) for L in llm.stack.layers]
    for L in llm.stack.layers:
        L.qkv.stream = L.o.stream = on
    return prev


def _restore(llm, prev):
    for L, (a, b) in zip(llm.stack.layers, prev):
        L.qkv.stream, L.o.stream = a, b


# ------------------------------------------------------------------ tiny config, the whole engine
FEED = [[7, 300], [12, 45], [99, 100], [5, 6]]


def _tiny_steps(eng, graph):
    """A system prompt for 2 sessions, then teacher-forced one-token text steps (the captured TextGraph, or eagerly).
    Returns the steps' hidden rows, the logits of the head on them, and the counters' rise per step."""
    kvs = [eng.system_role("<|im_start|>system\nYou are a helpful assistant.") for _ in range(2)]
    hids, lgs, rises = [], [], []
    try:
        for ids in FEED:
            before = _counts()
            _, hid = eng.text_step([(kv, [t]) for kv, t in zip(kvs, ids)], graph=graph)
            rises.append(tuple(a - b for a, b in zip(_counts(), before)))
            hids.append(hid.clone())
            lgs.append(eng.llm.lm_head(hid.clone()).clone())
    finally:
        for kv in kvs:
            kv.free()
    return torch.stack(hids), torch.stack(lgs), rises


def _drop_graphs(eng):
    for g in list(eng._tgraphs.values()):
        g.destroy()
    eng._tgraphs = {}


@pytest.mark.parametrize("fmt", FMTS)
def test_tiny_engine_projections_are_the_model_its_src_serves(dev, fmt):
    from fo import ops
    from fo.engine import FreezeOmniEngine
    from fo.ops import PackedLinear, PackedLinearW4, PackedLinearW8, PackedQKVQuant
    from fo.weights import FakeQuantSource
    A = FreezeOmniEngine(TINY, device=dev, max_sessions=4, attn_weights=fmt)
    P = FreezeOmniEngine(TINY, device=dev, max_sessions=4)                       # without the option
    assert A.attn_weights == fmt and P.attn_weights == "bf16" and not isinstance(P.src, FakeQuantSource)
    assert isinstance(A.src, FakeQuantSource) and (A.src.attn, A.src.fmt, A.src.lm_head) == (fmt, None, None)
    n = len(A.llm.stack.layers)
    # engine.src serves the CPU definition's W' of the four raw projection weights; everything else is unchanged
    for i in (0, n - 1):
        for p in PROJ:
            name = f"model.layers.{i}.self_attn.{p}.weight"
            raw = P.src.get(name, torch.bfloat16).cpu()
            want = _quantised(raw, fmt)
            assert torch.equal(A.src.get(name, torch.bfloat16).cpu().view(torch.int16), want.view(torch.int16)), name
            assert not torch.equal(want, raw)
        for name in (f"model.layers.{i}.self_attn.q_proj.bias", f"model.layers.{i}.mlp.down_proj.weight",
                     "model.embed_tokens.weight", "lm_head.weight"):
            assert torch.equal(A.src.get(name, torch.bfloat16), P.src.get(name, torch.bfloat16)), name
    # a bf16 engine on A.src: the same packed images
    B = FreezeOmniEngine(TINY, device=dev, max_sessions=4, source=A.src)
    o_cls = PackedLinearW8 if fmt == "fp8" else PackedLinearW4
    for LA, LB, LP in zip(A.llm.stack.layers, B.llm.stack.layers, P.llm.stack.layers):
        assert isinstance(LA.qkv, PackedQKVQuant) and LA.qkv.fmt == fmt and isinstance(LA.o, o_cls)
        assert LA.o.kind == "attn_o" and LA.o.stream_rows == 16 and LA.o.rows_rb == ()
        assert LA.qkv.stream == ops.ATTN_POLICY[fmt]["qkv"] and LA.o.stream == ops.ATTN_POLICY[fmt]["o"]
        assert type(LB.qkv) is PackedLinear and type(LB.o) is PackedLinear
        assert torch.equal(LA.qkv.packed, LB.qkv.packed) and torch.equal(LA.o.packed, LB.o.packed)
        assert torch.equal(LA.qkv.bias, LP.qkv.bias) and not torch.equal(LA.qkv.packed, LP.qkv.packed)
        assert type(LA.gu) is PackedLinear and type(LA.down) is PackedLinear
    codes = A.llm.attn_fp8_bytes if fmt == "fp8" else A.llm.attn_fp4_bytes
    assert codes > 0 and (A.llm.attn_fp8_bytes, A.llm.attn_fp4_bytes) == ((codes, 0) if fmt == "fp8" else (0, codes))
    assert (B.llm.attn_fp8_bytes, B.llm.attn_fp4_bytes) == (0, 0)
    assert A.llm.weight_bytes == P.llm.weight_bytes and A.llm.mlp_fp8_bytes == 0 and A.llm.mlp_fp4_bytes == 0
    # teacher-forced text steps, captured and eager, as shipped and with both GEMMs forced to stream: the counters rise
    # as the dispatch predicts (at capture only under the graph), the rows stay within the kernels' difference of B's
    for forced in (None, True):
        prev = _force(A.llm, True) if forced else None
        _drop_graphs(A)
        want = _predicted(fmt, n, forced, forced)
        try:
            for graph in (True, False):
                ha, la, ra = _tiny_steps(A, graph)
                hb, lb, rb = _tiny_steps(B, graph)
                assert ra == [want if (not graph or j == 0) else (0, 0, 0) for j in range(len(FEED))], (forced, graph, ra)
                assert all(r == (0, 0, 0) for r in rb), rb
                _close(ha, hb, "hidden rows against the bf16 engine on the same model")
                _close(la, lb, "logits against the bf16 engine on the same model")
        finally:
            _drop_graphs(A)
            if prev:
                _restore(A.llm, prev)
    # a 24-row prefill runs the images: bit-identical to B, whatever is forced
    ids = list(range(40, 64))
    prev = _force(A.llm, True)
    try:
        outs = []
        for eng in (A, B):
            kv = eng.llm.new_seq()
            try:
                before = _counts()
                h, _ = eng.llm.forward(eng.llm.embed(ids, round_fp16=True), [(kv, len(ids))])
                assert _counts() == before
                outs.append(h.clone())
            finally:
                kv.free()
        assert torch.equal(outs[0], outs[1])
    finally:
        _restore(A.llm, prev)
    # rebind_audiollm with new projection weights rebuilds the LLM with the option and re-wraps src the same way
    names = [f"model.layers.0.self_attn.{p}.weight" for p in PROJ]
    new = {k: (P.src.get(k, torch.bfloat16).float() * 0.5 + 0.01).to(torch.bfloat16).cpu() for k in names}
    assert A.rebind_audiollm(dict(new, **{"not.a.parameter": new[names[0]]})) == sorted(names)
    assert A.llm.attn_weights == fmt and isinstance(A.src, FakeQuantSource) and A.src.attn == fmt and A.src.fmt is None
    L0 = A.llm.stack.layers[0]
    assert isinstance(L0.qkv, PackedQKVQuant) and isinstance(L0.o, o_cls) and L0.o.kind == "attn_o"
    dq = {k: _quantised(v, fmt) for k, v in new.items()}
    for k in names:
        assert torch.equal(A.src.get(k, torch.bfloat16).cpu().view(torch.int16), dq[k].view(torch.int16)), k
    bias = torch.cat([P.src.get(f"model.layers.0.self_attn.{p}.bias") for p in PROJ[:3]])
    want = PackedLinear(torch.cat([dq[k] for k in names[:3]]).to(dev), bias, rope_hd=A.llm.hd)
    assert torch.equal(L0.qkv.packed, want.packed) and torch.equal(L0.qkv.bias, want.bias)
    assert torch.equal(L0.o.packed, PackedLinear(dq[names[3]].to(dev)).packed)
    for bad in ("int8", None):
        with pytest.raises(ValueError):
            FreezeOmniEngine(TINY, device=dev, max_sessions=4, attn_weights=bad)


@pytest.mark.parametrize("mlp", ["bf16", "mxfp4"])
@pytest.mark.parametrize("fmt", FMTS)
def test_12_rows_packed_activation_bookkeeping(dev, fmt, mlp):
    """9..16 rows write and read packed activations between the GEMMs (ops.XPack); a GEMM on the code stream reads fp32
    rows and writes none packed, so its neighbours must not expect them.  A 12-row forward over a bf16 MLP and over
    mlp_weights="mxfp4", with the policy as shipped and with q|k|v and o forced to stream, against the bf16 engine on
    the same model."""
    from fo.llm import LLMEngine
    from fo.weights import FakeQuantSource, SynthSource
    from oracle import configs
    from oracle.params import all_shapes
    cfg = configs.get("tiny")
    src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
    w4 = mlp == "mxfp4"
    A = LLMEngine(src, cfg["llm"], dev, kv_tokens=1024, attn_weights=fmt, mlp_weights="mxfp4" if w4 else "bf16")
    B = LLMEngine(FakeQuantSource(src, "mxfp4" if w4 else None, attn=fmt), cfg["llm"], dev, kv_tokens=1024)
    n = len(A.stack.layers)
    ids = list(range(30, 42))

    def run(eng):
        kv = eng.new_seq()
        try:
            before = _counts()
            h, _ = eng.forward(eng.embed(ids, round_fp16=True), [(kv, len(ids))])
            return h.clone(), tuple(a - b for a, b in zip(_counts(), before))
        finally:
            kv.free()

    hb, rb = run(B)
    assert rb == (0, 0, 0)
    for forced in (None, True):
        prev = _force(A, True) if forced else None
        try:
            ha, ra = run(A)
        finally:
            if prev:
                _restore(A, prev)
        want = _predicted(fmt, n, forced, forced)
        assert ra[0] == want[0] and ra[1] == want[1], (forced, ra, want)
        # (the general MXFP4 counter also counts the MXFP4 MLP's launches of that form)
        assert ra[2] >= want[2] and (w4 or ra[2] == want[2]), (forced, ra, want)
        assert torch.isfinite(ha).all()
        _close(ha, hb, f"12-row forward, forced={forced}")


def test_combinations_build_and_step(dev):
    from fo.engine import FreezeOmniEngine
    from fo.weights import FakeQuantSource
    for kw in (dict(attn_weights="fp8", mlp_weights="mxfp4", lm_head_weights="mxfp4", llm_kv="bf16"),
               dict(attn_weights="mxfp4", mlp_weights="mxfp4", lm_head_weights="fp8"),
               dict(attn_weights="mxfp4", llm_kv="bf16")):
        eng = FreezeOmniEngine(TINY, device=dev, max_sessions=4, **kw)
        assert isinstance(eng.src, FakeQuantSource) and eng.src.attn == kw["attn_weights"]
        assert eng.src.fmt == kw.get("mlp_weights") and eng.src.lm_head == kw.get("lm_head_weights")
        for forced in (False, True):
            prev = _force(eng.llm, True) if forced else None
            _drop_graphs(eng)
            for graph in (True, False):
                h, lg, _ = _tiny_steps(eng, graph)
                assert torch.isfinite(h).all() and torch.isfinite(lg).all()
            _drop_graphs(eng)
            if prev:
                _restore(eng.llm, prev)


# ------------------------------------------------------------------ two layers at real geometry
class _DeviceWeights(dict):
    """name -> np.float32 copy of a source's (device) weight, materialised on first use."""

    def __init__(self, src):
        super().__init__()
        self.src = src

    def __missing__(self, k):
        v = self.src.get(k).float().cpu().numpy()
        self[k] = v
        return v


def _limit(bound, control):
    """The bound where the control (the bf16 engine on the same W') meets it; twice the control's own distance where
    the control itself misses it on this W' (the rule of tests/test_mlp_mxfp4_gpu.py; both figures are printed, and
    recorded in DESIGN 5.9)."""
    return bound if control < bound else 2 * control


@pytest.mark.parametrize("fmt", FMTS)
def test_real_geometry_against_bf16_engine_and_oracle(dev, fmt):
    """Two Qwen2 layers at real geometry with q|k|v and o forced onto the code streams (so the kernels are exercised
    whatever ops.ATTN_POLICY ships): a 24-row prefill (the images: bit-identical to the bf16 engine on the same model),
    then 4 steps of 8 rows.  Against the bf16 engine on the same model 1e-3 abs + 1e-3 rel; against the numpy oracle on
    the same model the bounds of tests/test_full_depth_gpu.py (last hidden row abs < 1e-2, rel L2 < 2e-3, logits 5e-3
    abs + 5e-3 rel), the bf16 engine as the control.  Then a TextGraph at B = 8, captured once and replayed 3 times,
    against the eager path at top_k = 1."""
    from fo import ops
    from fo.engine import TextGraph
    from fo.llm import LLMEngine
    from fo.weights import FakeQuantSource, SynthSource
    from oracle import configs, nets
    from oracle.params import all_shapes
    cfg = configs.get("real")
    cfg["llm"]["num_hidden_layers"] = 2
    src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
    A = LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16, attn_weights=fmt)
    model = FakeQuantSource(src, None, attn=fmt)
    B = LLMEngine(model, cfg["llm"], dev, kv_tokens=4096, page_size=16)
    for LA, LB in zip(A.stack.layers, B.stack.layers):
        assert torch.equal(LA.qkv.packed, LB.qkv.packed) and torch.equal(LA.o.packed, LB.o.packed)
        assert LA.qkv.stream == ops.ATTN_POLICY[fmt]["qkv"] and LA.o.stream == ops.ATTN_POLICY[fmt]["o"]
    # the byte properties: per layer (4608 + 3584) x 3584 = 29,360,128 weights
    per = (4608 + 3584) * 3584
    assert per == 29360128
    if fmt == "fp8":
        assert A.attn_fp8_bytes == 2 * (per + (4608 + 3584) * 4) and A.attn_fp4_bytes == 0
    else:
        assert A.attn_fp4_bytes == 2 * (per // 2 + per // 32) and A.attn_fp8_bytes == 0
    assert (B.attn_fp8_bytes, B.attn_fp4_bytes) == (0, 0) and A.weight_bytes == B.weight_bytes
    assert A.mlp_fp8_bytes == 0 and A.mlp_fp4_bytes == 0
    _force(A, True)
    rng = np.random.default_rng(8)
    steps = [rng.integers(0, A.V, 24).tolist()] + [rng.integers(0, A.V, 8).tolist() for _ in range(4)]
    got = {}
    for name, eng in (("A", A), ("B", B)):
        kv = eng.new_seq()
        hs, lgs, xs = [], [], []
        try:
            for s, ids in enumerate(steps):
                x = eng.embed(ids, round_fp16=True)
                xs.append(x.cpu().numpy())
                before = _counts()
                h, bm = eng.forward(x, [(kv, len(ids))])
                want = _predicted(fmt, 2, True, True) if name == "A" and s > 0 else (0, 0, 0)
                assert tuple(a - b for a, b in zip(_counts(), before)) == want, (name, s)
                hs.append(h.clone())
                lgs.append(eng.logits(h, bm.last_rows_host).clone())
        finally:
            kv.free()
        got[name] = (hs, lgs, xs)
    for s in range(len(steps)):
        _close(got["A"][0][s], got["B"][0][s], f"step {s} hidden rows against the bf16 engine")
        _close(got["A"][1][s], got["B"][1][s], f"step {s} logits against the bf16 engine")
    assert torch.equal(got["A"][0][0], got["B"][0][0])          # the 24-row prefill ran the images
    # the oracle on the same model, the bf16 engine as the control
    W = _DeviceWeights(model)
    q = nets.Qwen2(W, cfg)
    okv = nets.KV(2)
    for s in range(len(steps)):
        h = q.forward(got["A"][2][s], okv)
        ref_lg = q.logits(h[-1:])[0]
        d = {}
        for name in ("A", "B"):
            hv = got[name][0][s][-1].float().cpu().numpy()
            lg = got[name][1][s][0].float().cpu().numpy()
            d[name] = (float(np.abs(hv - h[-1]).max()), float(np.linalg.norm(hv - h[-1]) / np.linalg.norm(h[-1])),
                       float((np.abs(lg - ref_lg) / (5e-3 + 5e-3 * np.abs(ref_lg))).max()))
        print(f"attn_weights={fmt} step {s}: against the oracle (last hidden row abs, rel L2, logits in units of 5e-3 "
              f"abs + 5e-3 rel): {fmt} {d['A']}, bf16 control {d['B']}")
        assert d["A"][0] < _limit(1e-2, d["B"][0]) and d["A"][1] < _limit(2e-3, d["B"][1]), (s, d)
        assert d["A"][2] <= _limit(1.0, d["B"][2]), (s, d)
    del W, q, okv
    # a TextGraph at B = 8, captured once and replayed 3 times, against the eager path at top_k = 1
    Bn = 8
    first = rng.integers(0, A.V, (Bn, 5)).tolist()
    feed0 = rng.integers(0, A.V, Bn).tolist()

    def sessions():
        seqs = [A.new_seq() for _ in range(Bn)]
        A.forward(A.embed([t for row in first for t in row], round_fp16=True), [(kv, 5) for kv in seqs])
        return seqs

    seqs = sessions()
    try:
        before = _counts()
        g = TextGraph(SimpleNamespace(device=dev, llm=A), Bn, 2048, 1, 0.0, 1.0, 0)
        want = _predicted(fmt, 2, True, True)
        assert tuple(a - b for a, b in zip(_counts(), before)) == want              # counted at capture
        try:
            feed, graph_ids = feed0, []
            for _ in range(3):
                feed, _ = g.run([(kv, [t]) for kv, t in zip(seqs, feed)])
                graph_ids.append(list(feed))
            assert tuple(a - b for a, b in zip(_counts(), before)) == want          # replays issue nothing new
        finally:
            g.destroy()
    finally:
        for kv in seqs:
            kv.free()
    seqs = sessions()
    try:
        feed, eager_ids = feed0, []
        for _ in range(3):
            h, bm = A.forward(A.embed(feed, round_fp16=True), [(kv, 1) for kv in seqs])
            ids = torch.empty(Bn, dtype=torch.int32, device=dev)
            ops.sample(A.logits(h, bm.last_rows_host), A.V, ids, torch.ones(Bn, dtype=torch.int32, device=dev))
            feed = ids.cpu().tolist()
            eager_ids.append(feed)
    finally:
        for kv in seqs:
            kv.free()
    assert graph_ids == eager_ids, (graph_ids, eager_ids)
    assert A.pool.pages_in_use() == 0


# ------------------------------------------------------------------ receive-only replica
@pytest.mark.parametrize("fmt", FMTS)
def test_receive_only_replica_gets_codes_scales_and_images(dev, fmt):
    """receive_weights=True allocates the projections' storages without quantising; fo.replica's walk finds them, so
    the copy of the frozen weights fills codes, scales and the bf16 images, and the replica computes the same bits."""
    from fo.engine import FreezeOmniEngine
    from fo.replica import copy_frozen, frozen_tensors
    from fo.weights import FakeQuantSource
    A = FreezeOmniEngine(TINY, device=dev, max_sessions=2, attn_weights=fmt)
    C = FreezeOmniEngine(TINY, device=dev, max_sessions=2, attn_weights=fmt, receive_weights=True)
    assert not isinstance(C.src, FakeQuantSource)
    assert (C.llm.attn_fp8_bytes, C.llm.attn_fp4_bytes) == (A.llm.attn_fp8_bytes, A.llm.attn_fp4_bytes)
    for eng in (A, C):
        ptrs = {t.data_ptr() for t in frozen_tensors(eng)}
        for L in eng.llm.stack.layers:
            for lin in (L.qkv, L.o):
                assert {lin.q.data_ptr(), lin.scales.data_ptr(), lin.packed.data_ptr()} <= ptrs
            assert L.qkv.bias.data_ptr() in ptrs
    assert copy_frozen(A, C) > A.llm.attn_fp8_bytes + A.llm.attn_fp4_bytes
    for LA, LC in zip(A.llm.stack.layers, C.llm.stack.layers):
        assert type(LC.qkv) is type(LA.qkv) and type(LC.o) is type(LA.o) and LC.o.kind == "attn_o"
        for a, c in ((LA.qkv, LC.qkv), (LA.o, LC.o)):
            assert torch.equal(a.q, c.q) and torch.equal(a.scales, c.scales) and torch.equal(a.packed, c.packed)
        assert torch.equal(LA.qkv.bias, LC.qkv.bias)
    ids = [5, 9, 200, 31, 77, 12]
    n = len(A.llm.stack.layers)
    outs = []
    for eng in (A, C):
        prev = _force(eng.llm, True)
        kv = eng.llm.new_seq()
        try:
            before = _counts()
            h, _ = eng.llm.forward(eng.llm.embed(ids, round_fp16=True), [(kv, len(ids))])
            assert tuple(x - y for x, y in zip(_counts(), before)) == _predicted(fmt, n, True, True)
            outs.append(h.clone())
        finally:
            kv.free()
            _restore(eng.llm, prev)
    assert torch.equal(outs[0], outs[1])
