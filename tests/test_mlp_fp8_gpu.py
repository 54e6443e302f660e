"""mlp_weights="fp8" through the engines: the option is a MODEL (the Qwen2 MLP weights become q * 2^e, served
dequantised by engine.src), not a per-launch approximation -- a bf16 engine built on the FP8 engine's src computes the
same thing to the accumulation-order difference between kernels, launches above 16 rows are bit-identical, and the
numpy oracle on the same src holds the FP8 engine to the full-depth bounds."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _w8_count():
    from fo import ops
    c = ops.launch_counts()
    return c["gemm_w8"] + c["gemm_w8_xs"]


def _close(a, b, what):
    a, b = (t.detach().float().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (a, b))
    np.testing.assert_allclose(a, b, atol=1e-3, rtol=1e-3, err_msg=what)


# ------------------------------------------------------------------ tiny config, the whole engine
def _tiny_flow(eng, dev, count):
    """System prompt, three one-chunk listens for 2 sessions, 6 teacher-forced text steps through the captured
    TextGraph.  Returns the state probabilities, the decision rows and the text steps' hidden rows."""
    from fo.speech import Framer
    nl = len(eng.llm.stack.layers)
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
        before = _w8_count()
        for j, ids in enumerate(feed):
            _, hid = eng.text_step([(kv, [t]) for kv, t in zip(kvs, ids)])
            hids.append(hid.clone())
            if j == 0 and count:   # the capture (counted when issued; every later step replays it)
                got = _w8_count() - before
                assert got >= 2 * nl and got % (2 * nl) == 0, got
        if count:
            assert _w8_count() - before == got   # replays issue nothing new
            before = _w8_count()
            eng.text_step([(kv, [t]) for kv, t in zip(kvs, [3, 4])], graph=False)
            assert _w8_count() - before == 2 * nl   # gate/up and down of every layer, per step
        else:
            assert _w8_count() == before
            eng.text_step([(kv, [t]) for kv, t in zip(kvs, [3, 4])], graph=False)
    finally:
        for kv in kvs:
            kv.free()
    return np.asarray(probs), torch.stack(rows), torch.stack(hids)


def test_tiny_engine_fp8_is_the_model_its_src_serves(dev):
    from fo import ops
    from fo.engine import FreezeOmniEngine
    from fo.ops import PackedLinear, PackedLinearW8
    from fo.weights import FakeQuantSource
    path = os.path.join(ROOT, "configs", "tiny")
    A = FreezeOmniEngine(path, device=dev, max_sessions=4, mlp_weights="fp8")
    assert isinstance(A.src, FakeQuantSource) and A.mlp_weights == "fp8"
    B = FreezeOmniEngine(path, device=dev, max_sessions=4, source=A.src)
    nl = len(A.llm.stack.layers)
    assert all(isinstance(L.gu, PackedLinearW8) and isinstance(L.down, PackedLinearW8) for L in A.llm.stack.layers)
    assert all(type(L.gu) is PackedLinear and type(L.down) is PackedLinear for L in B.llm.stack.layers)
    assert B.llm.mlp_fp8_bytes == 0 and A.llm.weight_bytes == B.llm.weight_bytes
    assert A.llm.mlp_fp8_bytes == sum(L.gu.fp8_nbytes + L.down.fp8_nbytes for L in A.llm.stack.layers) > 0
    for La, Lb in zip(A.llm.stack.layers, B.llm.stack.layers):      # one model: the same bf16 image in both engines
        assert torch.equal(La.gu.packed, Lb.gu.packed) and torch.equal(La.down.packed, Lb.down.packed)
    with pytest.raises(ValueError):
        FreezeOmniEngine(path, device=dev, max_sessions=4, mlp_weights="int8")
    pa, ra, ha = _tiny_flow(A, dev, True)
    pb, rb, hb = _tiny_flow(B, dev, False)
    np.testing.assert_allclose(pa, pb, atol=5e-4, rtol=0)
    _close(ra, rb, "listen decision rows")
    _close(ha, hb, "text step hidden rows")
    # a stage above 16 rows runs the bf16 image: bit-identical to B, no FP8 launch
    ids = list(range(1, 21))
    before = _w8_count()
    outs = []
    for eng in (A, B):
        kv = eng.llm.new_seq()
        try:
            h, _ = eng.llm.forward(eng.llm.embed(ids, round_fp16=True), [(kv, len(ids))])
            outs.append(h.clone())
        finally:
            kv.free()
    assert _w8_count() == before
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


def test_real_geometry_llm_fp8_against_bf16_engine_and_oracle(dev):
    """The fixture recipe of tests/test_real_qwen2_gpu.py with mlp_weights="fp8": a 24-row prefill (the bf16 image), then
    4 steps of 8 rows on fixed ids (gate/up on the X-stationary FP8 stream, down on the split-K form).  Against the
    bf16 engine on the same model: hidden rows and decision-row logits 1e-3 abs + 1e-3 rel; against the numpy oracle
    on the same model: the bounds of tests/test_full_depth_gpu.py."""
    from fo import ops
    from fo.llm import LLMEngine
    from fo.weights import FakeQuantSource, SynthSource
    from oracle import configs, nets
    from oracle.params import all_shapes
    cfg = configs.get("real")
    cfg["llm"]["num_hidden_layers"] = 2
    src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
    A = LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16, mlp_weights="fp8")
    model = FakeQuantSource(src)
    B = LLMEngine(model, cfg["llm"], dev, kv_tokens=4096, page_size=16)
    assert A.mlp_fp8_bytes == 2 * (3 * 18944 * 3584 + 4 * (2 * 18944 + 3584)) and B.mlp_fp8_bytes == 0
    assert A.weight_bytes == B.weight_bytes
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
                ops.launch_counts_reset()
                h, bm = eng.forward(x, [(kv, len(ids))])
                c = ops.launch_counts()
                want = (2, 2) if name == "A" and s > 0 else (0, 0)
                assert (c["gemm_w8"], c["gemm_w8_xs"]) == want, (name, s, c)
                hs.append(h.clone())
                lgs.append(eng.logits(h, bm.last_rows_host).clone())
        finally:
            kv.free()
        got[name] = (hs, lgs, xs)
    for s in range(len(steps)):
        _close(got["A"][0][s], got["B"][0][s], f"step {s} hidden rows, FP8 against the bf16 engine")
        _close(got["A"][1][s], got["B"][1][s], f"step {s} logits, FP8 against the bf16 engine")
    assert torch.equal(got["A"][0][0], got["B"][0][0])   # the 24-row prefill ran the same kernels on the same image
    # the oracle on the same model
    W = _DeviceWeights(model)
    q = nets.Qwen2(W, cfg)
    okv = nets.KV(2)
    for s in range(len(steps)):
        h = q.forward(got["A"][2][s], okv)
        hv = got["A"][0][s][-1].float().cpu().numpy()
        dh = float(np.abs(hv - h[-1]).max())
        rel = float(np.linalg.norm(hv - h[-1]) / np.linalg.norm(h[-1]))
        assert dh < 1e-2 and rel < 2e-3, (s, dh, rel)
        np.testing.assert_allclose(got["A"][1][s][0].float().cpu().numpy(), q.logits(h[-1:])[0], atol=5e-3, rtol=5e-3,
                                   err_msg=f"step {s} logits against the oracle")


def test_receive_only_replica_gets_codes_scales_and_image(dev):
    """receive_weights=True allocates the FP8 storages without quantising; fo.replica's walk finds them, so the copy
    of the frozen weights fills codes, scales and the bf16 image, and the replica computes the same bits."""
    from fo.engine import FreezeOmniEngine
    from fo.replica import copy_frozen, frozen_tensors
    from fo.weights import FakeQuantSource
    path = os.path.join(ROOT, "configs", "tiny")
    A = FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="fp8")
    C = FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="fp8", receive_weights=True)
    assert not isinstance(C.src, FakeQuantSource)
    ptrs = {t.data_ptr() for t in frozen_tensors(A)}
    for L in A.llm.stack.layers:
        for lin in (L.gu, L.down):
            assert {lin.q.data_ptr(), lin.scales.data_ptr(), lin.packed.data_ptr()} <= ptrs
    assert copy_frozen(A, C) > A.llm.mlp_fp8_bytes
    for La, Lc in zip(A.llm.stack.layers, C.llm.stack.layers):
        assert torch.equal(La.gu.q, Lc.gu.q) and torch.equal(La.down.scales, Lc.down.scales)
    ids = [5, 9, 200, 31, 77, 12]
    outs = []
    for eng in (A, C):
        kv = eng.llm.new_seq()
        try:
            before = _w8_count()
            h, _ = eng.llm.forward(eng.llm.embed(ids, round_fp16=True), [(kv, len(ids))])
            assert _w8_count() - before == 2 * len(eng.llm.stack.layers)
            outs.append(h.clone())
        finally:
            kv.free()
    assert torch.equal(outs[0], outs[1])
