"""mlp_weights="mxfp4" through the engines, mirroring tests/test_mlp_fp8_gpu.py: the option is a MODEL (the Qwen2 MLP
weights become q * 2^e with e2m1 codes and one e per 32-column block, served dequantised by engine.src), not a
per-launch approximation -- a bf16 engine built on the MXFP4 engine's src computes the same thing to the
accumulation-order difference between kernels, launches above 16 rows are bit-identical, and the numpy oracle on the
same src holds the MXFP4 engine to the full-depth bounds."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _policy():
    """(gate/up streams, down streams) at <= 16 rows: ops.W4_POLICY, the measured dispatch."""
    from fo import ops
    return int(bool(ops.W4_POLICY["gate_up"])), int(bool(ops.W4_POLICY["down"]))


def _w4_count():
    from fo import ops
    return sum(ops.w4_launch_counts().values())


def _w8_count():
    from fo import ops
    c = ops.launch_counts()
    return sum(c[k] for k in ("gemm_w8", "gemm_w8_xs", "gemm_w8_rows", "gemm_w8_rows128"))


def _close(a, b, what):
    a, b = (t.detach().float().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (a, b))
    np.testing.assert_allclose(a, b, atol=1e-3, rtol=1e-3, err_msg=what)


# ------------------------------------------------------------------ tiny config, the whole engine
def _tiny_flow(eng, dev, per_step):
    """System prompt, three one-chunk listens for 2 sessions, 6 teacher-forced text steps through the captured
    TextGraph.  per_step: the fo_gemm_w4 launches a <= 16-row step issues.  Returns the state probabilities, the
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
        before = _w4_count()
        got = 0
        for j, ids in enumerate(feed):
            _, hid = eng.text_step([(kv, [t]) for kv, t in zip(kvs, ids)])
            hids.append(hid.clone())
            if j == 0:   # the capture (counted when issued; every later step replays it)
                got = _w4_count() - before
                if per_step:
                    assert got >= per_step and got % per_step == 0, got
                else:
                    assert got == 0
        assert _w4_count() - before == got   # replays issue nothing new
        before = _w4_count()
        eng.text_step([(kv, [t]) for kv, t in zip(kvs, [3, 4])], graph=False)
        assert _w4_count() - before == per_step   # the dispatched GEMMs of every layer, per step
    finally:
        for kv in kvs:
            kv.free()
    return np.asarray(probs), torch.stack(rows), torch.stack(hids)


def test_tiny_engine_mxfp4_is_the_model_its_src_serves(dev):
    from fo.engine import FreezeOmniEngine
    from fo.ops import PackedLinear, PackedLinearW4
    from fo.weights import FakeQuantSource
    path = os.path.join(ROOT, "configs", "tiny")
    with pytest.raises(ValueError):
        FreezeOmniEngine(path, device=dev, max_sessions=4, mlp_weights="mxfp4", mlp_fp8_rows=64)
    A = FreezeOmniEngine(path, device=dev, max_sessions=4, mlp_weights="mxfp4")
    assert isinstance(A.src, FakeQuantSource) and A.src.fmt == "mxfp4" and A.mlp_weights == "mxfp4"
    B = FreezeOmniEngine(path, device=dev, max_sessions=4, source=A.src)
    nl = len(A.llm.stack.layers)
    assert all(isinstance(L.gu, PackedLinearW4) and isinstance(L.down, PackedLinearW4) for L in A.llm.stack.layers)
    assert all(type(L.gu) is PackedLinear and type(L.down) is PackedLinear for L in B.llm.stack.layers)
    assert A.llm.mlp_fp4_bytes == sum(L.gu.fp4_nbytes + L.down.fp4_nbytes for L in A.llm.stack.layers) > 0
    assert B.llm.mlp_fp4_bytes == 0 and A.llm.mlp_fp8_bytes == 0 and B.llm.mlp_fp8_bytes == 0
    assert A.llm.weight_bytes == B.llm.weight_bytes
    for La, Lb in zip(A.llm.stack.layers, B.llm.stack.layers):      # one model: the same bf16 image in both engines
        assert torch.equal(La.gu.packed, Lb.gu.packed) and torch.equal(La.down.packed, Lb.down.packed)
    w8_before = _w8_count()
    pa, ra, ha = _tiny_flow(A, dev, sum(_policy()) * nl)
    pb, rb, hb = _tiny_flow(B, dev, 0)
    assert _w8_count() == w8_before
    np.testing.assert_allclose(pa, pb, atol=5e-4, rtol=0)
    _close(ra, rb, "listen decision rows")
    _close(ha, hb, "text step hidden rows")
    # a stage above 16 rows runs the bf16 image: bit-identical to B, no MXFP4 launch
    ids = list(range(1, 21))
    before = _w4_count()
    outs = []
    for eng in (A, B):
        kv = eng.llm.new_seq()
        try:
            h, _ = eng.llm.forward(eng.llm.embed(ids, round_fp16=True), [(kv, len(ids))])
            outs.append(h.clone())
        finally:
            kv.free()
    assert _w4_count() == before
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
    where the control itself misses it on this W' (both figures are printed, and recorded in DESIGN 5.7)."""
    return bound if control < bound else 2 * control


def test_real_geometry_llm_mxfp4_against_bf16_engine_and_oracle(dev):
    """The fixture recipe of tests/test_real_qwen2_gpu.py with mlp_weights="mxfp4": a 24-row prefill (the bf16 image), then
    4 steps of 8 rows on fixed ids (the GEMMs of ops.W4_POLICY on the MXFP4 stream: gate/up X-stationary, down split-K).
    Against the bf16 engine on the same model: hidden rows and decision-row logits 1e-3 abs + 1e-3 rel; against the
    numpy oracle on the same model: the bounds of tests/test_full_depth_gpu.py (last hidden row abs < 1e-2, rel L2 <
    2e-3, logits 5e-3), with the bf16 engine on the same W' as the control."""
    from fo import ops
    from fo.llm import LLMEngine
    from fo.weights import FakeQuantSource, SynthSource
    from oracle import configs, nets
    from oracle.params import all_shapes
    cfg = configs.get("real")
    cfg["llm"]["num_hidden_layers"] = 2
    src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
    A = LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16, mlp_weights="mxfp4")
    model = FakeQuantSource(src, "mxfp4")
    B = LLMEngine(model, cfg["llm"], dev, kv_tokens=4096, page_size=16)
    assert A.mlp_fp4_bytes == 2 * (3 * 18944 * 3584 // 2 + 3 * 18944 * 3584 // 32)
    assert B.mlp_fp4_bytes == 0 and A.mlp_fp8_bytes == 0 and A.weight_bytes == B.weight_bytes
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
                ops.w4_launch_counts_reset()
                h, bm = eng.forward(x, [(kv, len(ids))])
                c = ops.w4_launch_counts()
                want = (0, 2 * gu, 2 * down) if name == "A" and s > 0 else (0, 0, 0)
                assert (c["w4"], c["w4_xs"], c["w4_sk"]) == want, (name, s, c)
                hs.append(h.clone())
                lgs.append(eng.logits(h, bm.last_rows_host).clone())
        finally:
            kv.free()
        got[name] = (hs, lgs, xs)
    for s in range(len(steps)):
        _close(got["A"][0][s], got["B"][0][s], f"step {s} hidden rows, MXFP4 against the bf16 engine")
        _close(got["A"][1][s], got["B"][1][s], f"step {s} logits, MXFP4 against the bf16 engine")
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
              f"mxfp4 {d['A']}, bf16 control {d['B']}")
        assert d["A"][0] < _limit(1e-2, d["B"][0]) and d["A"][1] < _limit(2e-3, d["B"][1]), (s, d)
        assert d["A"][2] <= _limit(1.0, d["B"][2]), (s, d)


def test_receive_only_replica_gets_codes_scales_and_image(dev):
    """receive_weights=True allocates the MXFP4 storages without quantising; fo.replica's walk finds them, so the copy
    of the frozen weights fills codes, scales and the bf16 image, and the replica computes the same bits."""
    from fo.engine import FreezeOmniEngine
    from fo.replica import copy_frozen, frozen_tensors
    from fo.weights import FakeQuantSource
    path = os.path.join(ROOT, "configs", "tiny")
    A = FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="mxfp4")
    C = FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="mxfp4", receive_weights=True)
    assert not isinstance(C.src, FakeQuantSource) and C.llm.mlp_fp4_bytes == A.llm.mlp_fp4_bytes
    for eng in (A, C):
        ptrs = {t.data_ptr() for t in frozen_tensors(eng)}
        for L in eng.llm.stack.layers:
            for lin in (L.gu, L.down):
                assert {lin.q.data_ptr(), lin.scales.data_ptr(), lin.packed.data_ptr()} <= ptrs
    assert copy_frozen(A, C) > A.llm.mlp_fp4_bytes
    for La, Lc in zip(A.llm.stack.layers, C.llm.stack.layers):
        assert torch.equal(La.gu.q, Lc.gu.q) and torch.equal(La.gu.scales, Lc.gu.scales)
        assert torch.equal(La.down.q, Lc.down.q) and torch.equal(La.down.scales, Lc.down.scales)
        assert torch.equal(La.gu.packed, Lc.gu.packed) and torch.equal(La.down.packed, Lc.down.packed)
    ids = [5, 9, 200, 31, 77, 12]
    outs = []
    for eng in (A, C):
        kv = eng.llm.new_seq()
        try:
            before = _w4_count()
            h, _ = eng.llm.forward(eng.llm.embed(ids, round_fp16=True), [(kv, len(ids))])
            assert _w4_count() - before == sum(_policy()) * len(eng.llm.stack.layers)
            outs.append(h.clone())
        finally:
            kv.free()
    assert torch.equal(outs[0], outs[1])
