"""mlp_weights="mxfp6" and lm_head_weights="mxfp6" through the engines, case for case as tests/test_mlp_mxfp4_gpu.py and
the MXFP4 head's engine tests: the option is a MODEL (the weights become q * 2^e with e2m3 codes and one e per
32-column block, served dequantised by engine.src), not a per-launch approximation -- a bf16 engine built on the MXFP6
engine's src computes the same thing to the accumulation-order difference between kernels, launches above 16 rows are
bit-identical, and the numpy oracle on the same src holds the MXFP6 engine to the full-depth bounds."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "configs", "tiny")


def _policy():
    """(gate/up streams, down streams) at <= 16 rows: ops.W6_POLICY, the measured dispatch."""
    from fo import ops
    return int(bool(ops.W6_POLICY["gate_up"])), int(bool(ops.W6_POLICY["down"]))


def _w6_count():
    """fo_gemm_w6 launches of the three MLP forms (the head's slot is the head tests')."""
    from fo import ops
    c = ops.w6_launch_counts()
    return c["w6"] + c["w6_xs"] + c["w6_sk"]


def _other_counts():
    """Every other quantised stream's launches: FP8, MXFP4 and the two older heads."""
    from fo import ops
    c = ops.launch_counts()
    return (sum(c[k] for k in ("gemm_w8", "gemm_w8_xs", "gemm_w8_rows", "gemm_w8_rows128")),
            sum(ops.w4_launch_counts().values()), sum(ops.head_launch_counts().values()))


def _close(a, b, what):
    a, b = (t.detach().float().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (a, b))
    np.testing.assert_allclose(a, b, atol=1e-3, rtol=1e-3, err_msg=what)


# ------------------------------------------------------------------ tiny config, the whole engine
def _tiny_flow(eng, dev, per_step):
    """System prompt, three one-chunk listens for 2 sessions, 6 teacher-forced text steps through the captured
    TextGraph.  per_step: the fo_gemm_w6 launches a <= 16-row step issues.  Returns the state probabilities, the
    decision rows and the text steps' hidden rows."""
    from fo.speech import Framer
    rng = np.random.default_rng(0)
    pcm = (rng.standard_normal((2, 2560 * 3)) * 0.05).astype(np.float32)
    kvs = [eng.system_role("<|im_start|>system\nYou are a helpful assistant.") for _ in range(2)]
    frs, fb = [Framer("A"), Framer("A")], eng.fbank("A")
    st = [dict(enc_cache=None, ada_cache=None, pe_index=0) for _ in range(2)]
    probs, rows, hids = [], [], []
    try:
        for c in range(3):
            items = []
            for b in range(2):
                w, first = frs[b].push(pcm[b, c * 2560:(c + 1) * 2560])
                items.append(dict(identity="user", status="ipu_sl" if c == 0 else "ipu_cl", feats=fb(w[None], [first])[0],
                                  kv=kvs[b], **st[b]))
            res = eng.listen(items)
            for b, r in enumerate(res):
                st[b] = dict(enc_cache=r["enc_cache"], ada_cache=r["ada_cache"], pe_index=r["pe_index"])
                probs.append((r["probs"]["state_1"], r["probs"]["state_2"]))
                rows.append(r["hidden_row"][0][r["hidden_row"][1]].clone())
        feed = [[7, 300], [12, 45], [99, 100], [5, 6], [200, 201], [31, 17]]
        before = _w6_count()
        got = 0
        for j, ids in enumerate(feed):
            _, hid = eng.text_step([(kv, [t]) for kv, t in zip(kvs, ids)])
            hids.append(hid.clone())
            if j == 0:   # the capture (counted when issued; every later step replays it)
                got = _w6_count() - before
                if per_step:
                    assert got >= per_step and got % per_step == 0, got
                else:
                    assert got == 0
        assert _w6_count() - before == got   # replays issue nothing new
        before = _w6_count()
        eng.text_step([(kv, [t]) for kv, t in zip(kvs, [3, 4])], graph=False)
        assert _w6_count() - before == per_step   # the dispatched GEMMs of every layer, per step
    finally:
        for kv in kvs:
            kv.free()
    return np.asarray(probs), torch.stack(rows), torch.stack(hids)


def test_tiny_engine_mxfp6_is_the_model_its_src_serves(dev):
    from fo.engine import FreezeOmniEngine
    from fo.ops import PackedLinear, PackedLinearW6
    from fo.quant import quantize_blocks_e2m3
    from fo.weights import FakeQuantSource
    for bad in (dict(mlp_fp8_rows=64), dict(mlp_mxfp4_rows=64), dict(attn_weights="mxfp6")):
        with pytest.raises(ValueError):
            FreezeOmniEngine(TINY, device=dev, max_sessions=4, mlp_weights="mxfp6", **bad)
    A = FreezeOmniEngine(TINY, device=dev, max_sessions=4, mlp_weights="mxfp6")
    P = FreezeOmniEngine(TINY, device=dev, max_sessions=4)
    assert isinstance(A.src, FakeQuantSource) and A.src.fmt == "mxfp6" and A.mlp_weights == "mxfp6"
    # engine.src serves the CPU definition's W' of the raw weight
    name = "model.layers.0.mlp.down_proj.weight"
    raw = P.src.get(name, torch.bfloat16).cpu()
    want = quantize_blocks_e2m3(raw)[2]
    assert torch.equal(A.src.get(name, torch.bfloat16).cpu().view(torch.int16), want.view(torch.int16))
    assert not torch.equal(want, raw)
    B = FreezeOmniEngine(TINY, device=dev, max_sessions=4, source=A.src)
    nl = len(A.llm.stack.layers)
    assert all(isinstance(L.gu, PackedLinearW6) and isinstance(L.down, PackedLinearW6) for L in A.llm.stack.layers)
    assert all(type(L.gu) is PackedLinear and type(L.down) is PackedLinear for L in B.llm.stack.layers)
    assert A.llm.mlp_fp6_bytes == sum(L.gu.fp6_nbytes + L.down.fp6_nbytes for L in A.llm.stack.layers) > 0
    assert B.llm.mlp_fp6_bytes == 0 and A.llm.mlp_fp8_bytes == 0 and A.llm.mlp_fp4_bytes == 0
    assert A.llm.lm_head_fp6_bytes == 0 and A.llm.weight_bytes == B.llm.weight_bytes == P.llm.weight_bytes
    for La, Lb in zip(A.llm.stack.layers, B.llm.stack.layers):      # one model: the same bf16 image in both engines
        assert torch.equal(La.gu.packed, Lb.gu.packed) and torch.equal(La.down.packed, Lb.down.packed)
    others = _other_counts()
    pa, ra, ha = _tiny_flow(A, dev, sum(_policy()) * nl)
    pb, rb, hb = _tiny_flow(B, dev, 0)
    assert _other_counts() == others
    np.testing.assert_allclose(pa, pb, atol=5e-4, rtol=0)
    _close(ra, rb, "listen decision rows")
    _close(ha, hb, "text step hidden rows")
    # a stage above 16 rows runs the bf16 image: bit-identical to B, no MXFP6 launch
    ids = list(range(1, 21))
    before = _w6_count()
    outs = []
    for eng in (A, B):
        kv = eng.llm.new_seq()
        try:
            h, _ = eng.llm.forward(eng.llm.embed(ids, round_fp16=True), [(kv, len(ids))])
            outs.append(h.clone())
        finally:
            kv.free()
    assert _w6_count() == before
    assert torch.equal(outs[0], outs[1])


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
    """The issue's bound where the control (the bf16 engine on the same W') meets it; twice the control's own distance
    where the control itself misses it on this W' (the rule of tests/test_mlp_mxfp4_gpu.py; both figures are printed)."""
    return bound if control < bound else 2 * control


def _real(dev):
    from fo.weights import SynthSource
    from oracle import configs
    from oracle.params import all_shapes
    cfg = configs.get("real")
    cfg["llm"]["num_hidden_layers"] = 2
    return cfg, SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])


def test_real_geometry_llm_mxfp6_against_bf16_engine_and_oracle(dev):
    """The fixture recipe of tests/test_real_qwen2_gpu.py with mlp_weights="mxfp6": a 24-row prefill (the bf16 image), then
    4 steps of 8 rows on fixed ids (the GEMMs of ops.W6_POLICY on the MXFP6 stream: gate/up X-stationary, down split-K).
    Against the bf16 engine on the same model: hidden rows and decision-row logits 1e-3 abs + 1e-3 rel; against the
    numpy oracle on the same model: the bounds of tests/test_full_depth_gpu.py (last hidden row abs < 1e-2, rel L2 <
    2e-3, logits 5e-3), with the bf16 engine on the same W' as the control."""
    from fo import ops
    from fo.llm import LLMEngine
    from fo.weights import FakeQuantSource
    from oracle import nets
    cfg, src = _real(dev)
    A = LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16, mlp_weights="mxfp6")
    model = FakeQuantSource(src, "mxfp6")
    B = LLMEngine(model, cfg["llm"], dev, kv_tokens=4096, page_size=16)
    assert A.mlp_fp6_bytes == 2 * (3 * 18944 * 3584 * 3 // 4 + 3 * 18944 * 3584 // 32)      # 6.25 bits per weight
    assert B.mlp_fp6_bytes == 0 and A.mlp_fp8_bytes == 0 and A.mlp_fp4_bytes == 0 and A.weight_bytes == B.weight_bytes
    gu, down = _policy()
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
                ops.w6_launch_counts_reset()
                h, bm = eng.forward(x, [(kv, len(ids))])
                c = ops.w6_launch_counts()
                want = (0, 2 * gu, 2 * down, 0) if name == "A" and s > 0 else (0, 0, 0, 0)
                assert (c["w6"], c["w6_xs"], c["w6_sk"], c["w6_head"]) == want, (name, s, c)
                hs.append(h.clone())
                lgs.append(eng.logits(h, bm.last_rows_host).clone())
        finally:
            kv.free()
        got[name] = (hs, lgs, xs)
    for s in range(len(steps)):
        _close(got["A"][0][s], got["B"][0][s], f"step {s} hidden rows, MXFP6 against the bf16 engine")
        _close(got["A"][1][s], got["B"][1][s], f"step {s} logits, MXFP6 against the bf16 engine")
    assert torch.equal(got["A"][0][0], got["B"][0][0])   # the 24-row prefill ran the same kernels on the same image
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
        print(f"step {s}: against the oracle (last hidden row abs, rel L2, logits in units of 5e-3 abs + 5e-3 rel): "
              f"mxfp6 {d['A']}, bf16 control {d['B']}")
        assert d["A"][0] < _limit(1e-2, d["B"][0]) and d["A"][1] < _limit(2e-3, d["B"][1]), (s, d)
        assert d["A"][2] <= _limit(1.0, d["B"][2]), (s, d)


def test_receive_only_replica_gets_codes_scales_and_image(dev):
    """receive_weights=True allocates the MXFP6 storages (MLP and head) without quantising; fo.replica's walk finds
    them, so the copy of the frozen weights fills codes, scales and the bf16 image, and the replica computes the same
    bits."""
    from fo.engine import FreezeOmniEngine
    from fo.replica import copy_frozen, frozen_tensors
    from fo.weights import FakeQuantSource
    kw = dict(device=dev, max_sessions=2, mlp_weights="mxfp6", lm_head_weights="mxfp6")
    A = FreezeOmniEngine(TINY, **kw)
    C = FreezeOmniEngine(TINY, receive_weights=True, **kw)
    assert not isinstance(C.src, FakeQuantSource) and C.llm.mlp_fp6_bytes == A.llm.mlp_fp6_bytes > 0
    assert C.llm.lm_head_fp6_bytes == A.llm.lm_head_fp6_bytes > 0 and type(C.llm.lm_head) is type(A.llm.lm_head)
    for eng in (A, C):
        ptrs = {t.data_ptr() for t in frozen_tensors(eng)}
        for lin in [eng.llm.lm_head] + [l for L in eng.llm.stack.layers for l in (L.gu, L.down)]:
            assert {lin.q.data_ptr(), lin.scales.data_ptr(), lin.packed.data_ptr()} <= ptrs
    assert copy_frozen(A, C) > A.llm.mlp_fp6_bytes + A.llm.lm_head_fp6_bytes
    for La, Lc in zip(A.llm.stack.layers, C.llm.stack.layers):
        assert torch.equal(La.gu.q, Lc.gu.q) and torch.equal(La.gu.scales, Lc.gu.scales)
        assert torch.equal(La.down.q, Lc.down.q) and torch.equal(La.down.scales, Lc.down.scales)
        assert torch.equal(La.gu.packed, Lc.gu.packed) and torch.equal(La.down.packed, Lc.down.packed)
    a, c = A.llm.lm_head, C.llm.lm_head
    assert torch.equal(a.q, c.q) and torch.equal(a.scales, c.scales) and torch.equal(a.packed, c.packed)
    ids = [5, 9, 200, 31, 77, 12]
    outs = []
    for eng in (A, C):
        kv = eng.llm.new_seq()
        try:
            before = _w6_count()
            h, _ = eng.llm.forward(eng.llm.embed(ids, round_fp16=True), [(kv, len(ids))])
            assert _w6_count() - before == sum(_policy()) * len(eng.llm.stack.layers)
            before = _w6_count()
            lg = eng.llm.logits(h, list(range(len(ids))))
            assert _w6_count() - before == 1        # the tiny head (K = 128): the general plain form
            outs.append((h.clone(), lg.clone()))
        finally:
            kv.free()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------ lm_head_weights="mxfp6"
FEED = [[7, 300], [12, 45], [99, 100], [5, 6]]


def _head_counts():
    """(fo_gemm_w6_head launches, fo_gemm_w6 general-form launches)."""
    from fo import ops
    c = ops.w6_launch_counts()
    return c["w6_head"], c["w6"]


def _tiny_steps(eng, graph):
    """A system prompt for 2 sessions, then teacher-forced one-token text steps (the captured TextGraph, or eagerly).
    Returns the steps' hidden rows, the logits of the head on them, and the counters' rise per step."""
    kvs = [eng.system_role("<|im_start|>system\nYou are a helpful assistant.") for _ in range(2)]
    hids, lgs, rises = [], [], []
    try:
        for ids in FEED:
            before = _head_counts()
            _, hid = eng.text_step([(kv, [t]) for kv, t in zip(kvs, ids)], graph=graph)
            rises.append(tuple(a - b for a, b in zip(_head_counts(), before)))
            hids.append(hid.clone())
            lgs.append(eng.llm.lm_head(hid.clone()).clone())
    finally:
        for kv in kvs:
            kv.free()
    return torch.stack(hids), torch.stack(lgs), rises


def test_tiny_engine_head_is_the_model_its_src_serves(dev):
    from fo.engine import FreezeOmniEngine
    from fo.ops import PackedLinear, PackedLinearW6
    from fo.quant import quantize_blocks_e2m3
    from fo.weights import FakeQuantSource
    A = FreezeOmniEngine(TINY, device=dev, max_sessions=4, lm_head_weights="mxfp6")
    P = FreezeOmniEngine(TINY, device=dev, max_sessions=4)                       # without the option
    assert A.lm_head_weights == "mxfp6" and isinstance(A.src, FakeQuantSource)
    assert A.src.lm_head == "mxfp6" and A.src.fmt is None
    raw = P.src.get("lm_head.weight", torch.bfloat16)
    want = quantize_blocks_e2m3(raw.cpu())[2]
    assert torch.equal(A.src.get("lm_head.weight", torch.bfloat16).cpu().view(torch.int16), want.view(torch.int16))
    assert not torch.equal(want, raw.cpu())
    for name in ("model.embed_tokens.weight", "model.layers.0.mlp.down_proj.weight"):
        assert torch.equal(A.src.get(name, torch.bfloat16), P.src.get(name, torch.bfloat16))
    assert torch.equal(A.llm.embed_tokens, P.llm.embed_tokens)
    B = FreezeOmniEngine(TINY, device=dev, max_sessions=4, source=A.src)
    head = A.llm.lm_head
    assert isinstance(head, PackedLinearW6) and head.kind == "head"
    assert type(B.llm.lm_head) is PackedLinear and torch.equal(head.packed, B.llm.lm_head.packed)
    assert all(type(L.gu) is PackedLinear and type(L.down) is PackedLinear for L in A.llm.stack.layers)
    assert A.llm.lm_head_fp6_bytes == head.fp6_nbytes > 0 and B.llm.lm_head_fp6_bytes == 0
    assert (A.llm.lm_head_fp8_bytes, A.llm.lm_head_fp4_bytes, A.llm.mlp_fp6_bytes) == (0, 0, 0)
    assert A.llm.weight_bytes == P.llm.weight_bytes and head.nbytes == B.llm.lm_head.nbytes
    # the tiny head (K = 128) streams through the general plain form: one launch per step, counted at capture
    for graph in (True, False):
        ha, la, ra = _tiny_steps(A, graph)
        hp, _, rp = _tiny_steps(P, graph)
        hb, lb, _ = _tiny_steps(B, graph)
        assert ra == [(0, 1) if (not graph or j == 0) else (0, 0) for j in range(len(FEED))], ra
        assert all(r == (0, 0) for r in rp), rp
        assert torch.equal(ha, hp) and torch.equal(ha, hb)      # the head changes nothing upstream
        _close(la, lb, "logits against the bf16 engine on the same model")
    # rebind_audiollm with a new lm_head.weight rebuilds the LLM with the option and re-wraps src the same way
    raw2 = (raw.float() * 0.5 + 0.01).to(torch.bfloat16).cpu()
    assert A.rebind_audiollm({"lm_head.weight": raw2, "not.a.parameter": raw2}) == ["lm_head.weight"]
    want2 = quantize_blocks_e2m3(raw2)[2]
    assert type(A.llm.lm_head) is PackedLinearW6 and A.llm.lm_head.kind == "head" and A.llm.lm_head_weights == "mxfp6"
    assert isinstance(A.src, FakeQuantSource) and A.src.lm_head == "mxfp6" and A.src.fmt is None
    assert torch.equal(A.src.get("lm_head.weight", torch.bfloat16).cpu().view(torch.int16), want2.view(torch.int16))
    assert torch.equal(A.llm.lm_head.packed, PackedLinear(want2.to(dev)).packed)


def test_combinations_build_and_step(dev):
    """The new values beside every other option."""
    from fo.engine import FreezeOmniEngine
    from fo.weights import FakeQuantSource
    for kw in (dict(mlp_weights="mxfp6", lm_head_weights="fp8", attn_weights="mxfp4"),
               dict(mlp_weights="mxfp4", mlp_mxfp4_rows=64, lm_head_weights="mxfp6", llm_kv="bf16"),
               dict(mlp_weights="fp8", mlp_fp8_rows=64, lm_head_weights="mxfp6", attn_weights="fp8"),
               dict(mlp_weights="mxfp6", lm_head_weights="mxfp6")):
        eng = FreezeOmniEngine(TINY, device=dev, max_sessions=4, **kw)
        assert isinstance(eng.src, FakeQuantSource) and eng.src.lm_head == kw["lm_head_weights"]
        assert eng.src.fmt == kw["mlp_weights"]
        for graph in (True, False):
            h, lg, _ = _tiny_steps(eng, graph)
            assert torch.isfinite(h).all() and torch.isfinite(lg).all()


def test_real_geometry_head_against_bf16_engine_and_oracle(dev):
    """Two Qwen2 layers at real geometry under the full 152,064 x 3584 head: a 24-row prefill (logits of all 24 rows:
    the bf16 image, bit-identical to the bf16 engine on the same model), then 4 steps of 8 rows whose logits of all 8
    rows issue one fo_gemm_w6_head launch each where ops.W6_POLICY streams the head.  Against the bf16 engine on the
    same model 1e-3 abs + 1e-3 rel; against the numpy oracle on the same model the decision row's logits at 5e-3 abs +
    5e-3 rel (tests/test_full_depth_gpu.py), the bf16 engine as the control.  Then a TextGraph at B = 8, captured once
    and replayed 3 times, against the eager path at top_k = 1."""
    from fo import ops
    from fo.engine import TextGraph
    from fo.llm import LLMEngine
    from fo.weights import FakeQuantSource
    from oracle import nets
    cfg, src = _real(dev)
    A = LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16, lm_head_weights="mxfp6")
    model = FakeQuantSource(src, None, lm_head="mxfp6")
    B = LLMEngine(model, cfg["llm"], dev, kv_tokens=4096, page_size=16)
    V, D = 152064, 3584
    assert (A.V, A.D) == (V, D) and torch.equal(A.lm_head.packed, B.lm_head.packed)
    assert A.lm_head_fp6_bytes == V * D * 3 // 4 + V * D // 32 and A.lm_head_fp8_bytes == 0 and A.lm_head_fp4_bytes == 0
    assert A.weight_bytes == B.weight_bytes and A.mlp_fp6_bytes == 0
    streams = int(bool(ops.W6_POLICY["head"]))
    assert A.lm_head.streams(8) == bool(streams) and not A.lm_head.streams(24) and A.lm_head.stream_rows == 16
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
                h, _ = eng.forward(x, [(kv, len(ids))])
                hs.append(h.clone())
                before = _head_counts()
                lgs.append(eng.logits(h, list(range(len(ids)))).clone())
                want = (streams, 0) if name == "A" and s > 0 else (0, 0)
                assert tuple(a - b for a, b in zip(_head_counts(), before)) == want, (name, s)
        finally:
            kv.free()
        got[name] = (hs, lgs, xs)
    for s in range(len(steps)):
        assert torch.equal(got["A"][0][s], got["B"][0][s])      # nothing upstream of the head differs
        _close(got["A"][1][s], got["B"][1][s], f"step {s} logits against the bf16 engine")
    assert torch.equal(got["A"][1][0], got["B"][1][0])          # the 24-row prefill's logits ran the image
    W = _DeviceWeights(model)
    q = nets.Qwen2(W, cfg)
    okv = nets.KV(2)
    for s in range(len(steps)):
        h = q.forward(got["A"][2][s], okv)
        ref_lg = q.logits(h[-1:])[0]
        d = {}
        for name in ("A", "B"):
            lg = got[name][1][s][-1].float().cpu().numpy()
            d[name] = float((np.abs(lg - ref_lg) / (5e-3 + 5e-3 * np.abs(ref_lg))).max())
        print(f"lm_head_weights=mxfp6 step {s}: decision-row logits against the oracle in units of 5e-3 abs + 5e-3 rel: "
              f"mxfp6 head {d['A']:.4f}, bf16 control {d['B']:.4f}")
        assert d["A"] <= _limit(1.0, d["B"]), (s, d)
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
        before = _head_counts()
        g = TextGraph(SimpleNamespace(device=dev, llm=A), Bn, 2048, 1, 0.0, 1.0, 0)
        assert tuple(a - b for a, b in zip(_head_counts(), before)) == (streams, 0)      # counted at capture
        try:
            feed, graph_ids = feed0, []
            for _ in range(3):
                feed, _ = g.run([(kv, [t]) for kv, t in zip(seqs, feed)])
                graph_ids.append(list(feed))
            assert tuple(a - b for a, b in zip(_head_counts(), before)) == (streams, 0)  # replays issue nothing new
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
