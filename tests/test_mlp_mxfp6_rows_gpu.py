"""mlp_mxfp6_rows=64 through the engines (tests/test_mlp_mxfp4_rows_gpu.py's four tests on the MXFP6 option): Qwen2 steps
of 17..64 rows stream the MXFP6 codes (fo_gemm_w6_rows) for the GEMMs and row counts of ops.W6_ROWS_POLICY.  The model
does not change: a bf16 engine on the same (dequantised) weights agrees to the accumulation-order difference between
kernels, and the numpy oracle on the same model holds the engine to the full-depth bounds (through
tests/test_mlp_mxfp6_gpu.py's _limit, the bf16 engine on the same W' as the control).  Steps of <= 16 rows and > 64 rows
dispatch exactly as under mlp_mxfp6_rows=16."""
import os

import numpy as np
import pytest
import torch

from test_mlp_mxfp6_gpu import _DeviceWeights, _close, _limit, _policy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows_count():
    from fo import ops
    return ops.w6_rows_launch_count()


def _per_forward(stack, T):
    """fo_gemm_w6_rows calls of one T-row forward under the layers' dispatch (ops.W6_ROWS_POLICY, or every pair where
    that is empty and the test forced them, through PackedLinearW6.streams)."""
    if T <= 16:
        return 0
    return sum(int(L.gu.streams(T)) + int(L.down.streams(T)) for L in stack.layers)


def _force_if_policy_is_empty(stack):
    """Were every (GEMM, row blocks) pair left on the image, the kernels would still be covered: rows_rb is the
    PackedLinearW6 attribute that sends every 17..64-row call to them."""
    from fo import ops
    if not any(ops.W6_ROWS_POLICY.values()):
        for L in stack.layers:
            L.gu.rows_rb = L.down.rows_rb = (2, 3, 4)


# ------------------------------------------------------------------ two layers at real geometry
def test_real_geometry_duplex_shapes_against_bf16_engine_and_oracle(dev):
    """Eight sessions; steps of 8 x 3, 4, 5, 6 and 8 tokens (24..64 rows: the duplex tick shapes), then 8 x 1 (the
    <= 16-row kernels) and 8 x 9 = 72 rows on fresh sessions (the image: bit-equal to the bf16 engine).  The oracle
    follows session 0 (and a fresh cache for the 72-row step)."""
    from fo import ops
    from fo.llm import LLMEngine
    from fo.weights import FakeQuantSource, SynthSource
    from oracle import configs, nets
    from oracle.params import all_shapes
    cfg = configs.get("real")
    cfg["llm"]["num_hidden_layers"] = 2
    src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
    A = LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16, mlp_weights="mxfp6", mlp_rows=64)
    model = FakeQuantSource(src, "mxfp6")
    B = LLMEngine(model, cfg["llm"], dev, kv_tokens=4096, page_size=16)
    _force_if_policy_is_empty(A.stack)
    assert A.weight_bytes == B.weight_bytes and A.stack.mlp_rows == 64 and A.stack.mlp_weights == "mxfp6"
    assert all(L.gu.stream_rows == 64 and L.down.stream_rows == 64 for L in A.stack.layers)
    gu, down = _policy()
    S = 8
    per = [3, 4, 5, 6, 8, 1, 9]
    rng = np.random.default_rng(8)
    steps = [rng.integers(0, A.V, S * n).tolist() for n in per]
    got = {}
    for name, eng in (("A", A), ("B", B)):
        kvs = [eng.new_seq() for _ in range(S)]
        hs, lgs, xs = [], [], []
        try:
            for n, ids in zip(per, steps):
                x = eng.embed(ids, round_fp16=True)
                xs.append(x[:n].cpu().numpy())   # session 0's rows come first
                if S * n > 64:   # fresh sessions: no history from the MXFP6 steps, so A and B compute equal bits
                    kvs += [eng.new_seq() for _ in range(S)]
                ops.w6_launch_counts_reset()
                h, bm = eng.forward(x, [(kv, n) for kv in kvs[-S:]])
                c = ops.w6_launch_counts()
                T = S * n
                if name == "B" or T > 64:
                    want = (0, 0, 0, 0)
                elif T <= 16:
                    want = (0, 0, 2 * gu, 2 * down)
                else:
                    want = (_per_forward(A.stack, T), 0, 0, 0)
                    assert want[0] > 0
                assert (_rows_count(), c["w6"], c["w6_xs"], c["w6_sk"]) == want, (name, T, c, _rows_count())
                hs.append(h.clone())
                lgs.append(eng.logits(h, bm.last_rows_host).clone())
        finally:
            for kv in kvs:
                kv.free()
        got[name] = (hs, lgs, xs)
    for s, n in enumerate(per):
        _close(got["A"][0][s], got["B"][0][s], f"{S} x {n} rows: hidden rows, MXFP6 against the bf16 engine")
        _close(got["A"][1][s], got["B"][1][s], f"{S} x {n} rows: logits, MXFP6 against the bf16 engine")
    assert torch.equal(got["A"][0][-1], got["B"][0][-1])   # 72 rows: the same kernels on the same image
    # the oracle on the same model, session 0, the bf16 engine as the control
    W = _DeviceWeights(model)
    q = nets.Qwen2(W, cfg)
    okv = nets.KV(2)
    for s, n in enumerate(per):
        if S * n > 64:
            okv = nets.KV(2)
        h = q.forward(got["A"][2][s], okv)
        ref_lg = q.logits(h[-1:])[0]
        d = {}
        for name in ("A", "B"):
            hv = got[name][0][s][n - 1].float().cpu().numpy()
            lg = got[name][1][s][0].float().cpu().numpy()
            d[name] = (float(np.abs(hv - h[-1]).max()), float(np.linalg.norm(hv - h[-1]) / np.linalg.norm(h[-1])),
                       float((np.abs(lg - ref_lg) / (5e-3 + 5e-3 * np.abs(ref_lg))).max()))
        print(f"{S} x {n} rows: against the oracle (last hidden row abs, rel L2, logits in units of 5e-3 abs + 5e-3 "
              f"rel): mxfp6 {d['A']}, bf16 control {d['B']}")
        assert d["A"][0] < _limit(1e-2, d["B"][0]) and d["A"][1] < _limit(2e-3, d["B"][1]), (s, d)
        assert d["A"][2] <= _limit(1.0, d["B"][2]), (s, d)


# ------------------------------------------------------------------ tiny config, the whole engine
def _listen_flow(eng, n_sess):
    """System prompt, then three one-chunk listens of n_sess sessions (2 tokens each from the second chunk on).
    Returns (state probabilities, decision rows) and the fo_gemm_w6_rows calls of each listen."""
    from fo.speech import Framer
    rng = np.random.default_rng(0)
    pcm = (rng.standard_normal((n_sess, 2560 * 3)) * 0.05).astype(np.float32)
    kvs = [eng.system_role("<|im_start|>system\nYou are a helpful assistant.") for _ in range(n_sess)]
    frs, fb = [Framer("A") for _ in range(n_sess)], eng.fbank("A")
    st = [dict(enc_cache=None, ada_cache=None, pe_index=0) for _ in range(n_sess)]
    probs, rows, launches = [], [], []
    try:
        for c in range(3):
            items = []
            for b in range(n_sess):
                w, first = frs[b].push(pcm[b, c * 2560:(c + 1) * 2560])
                items.append(dict(identity="user", status="ipu_sl" if c == 0 else "ipu_cl",
                                  feats=fb(w[None], [first])[0], kv=kvs[b], **st[b]))
            before = _rows_count()
            res = eng.listen(items)
            launches.append(_rows_count() - before)
            for b, r in enumerate(res):
                st[b] = dict(enc_cache=r["enc_cache"], ada_cache=r["ada_cache"], pe_index=r["pe_index"])
                probs.append((r["probs"]["state_1"], r["probs"]["state_2"]))
                rows.append(r["hidden_row"][0][r["hidden_row"][1]].clone())
    finally:
        for kv in kvs:
            kv.free()
    return np.asarray(probs), torch.stack(rows), launches


def _prefill(eng, ids):
    kv = eng.llm.new_seq()
    try:
        before = _rows_count()
        h, _ = eng.llm.forward(eng.llm.embed(ids, round_fp16=True), [(kv, len(ids))])
        return h.clone(), _rows_count() - before
    finally:
        kv.free()


def test_tiny_engine_streams_17_to_64_rows(dev):
    from fo.engine import FreezeOmniEngine
    path = os.path.join(ROOT, "configs", "tiny")
    A = FreezeOmniEngine(path, device=dev, max_sessions=12, mlp_weights="mxfp6", mlp_mxfp6_rows=64)
    assert A.mlp_mxfp6_rows == 64 and A.llm.stack.mlp_rows == 64 and A.mlp_fp8_rows == 16 and A.mlp_mxfp4_rows == 16
    assert A.llm.stack.mlp_weights == "mxfp6"
    B = FreezeOmniEngine(path, device=dev, max_sessions=12, source=A.src)
    assert B.mlp_mxfp6_rows == 16
    _force_if_policy_is_empty(A.llm.stack)
    nl = len(A.llm.stack.layers)
    # a 20-token prefill: eager, every layer's policy pairs on the new kernel
    ids = list(range(1, 21))
    want = _per_forward(A.llm.stack, 20)
    (ha, na), (hb, nb) = _prefill(A, ids), _prefill(B, ids)
    assert na == want and nl <= want <= 2 * nl and nb == 0
    _close(ha, hb, "20-row prefill, MXFP6 against the bf16 engine")
    # one-chunk listens of 10 sessions: 20 rows through the captured listen graph
    pa, ra, la = _listen_flow(A, 10)
    pa2, ra2, la2 = _listen_flow(A, 10)
    pb, rb, lb = _listen_flow(B, 10)
    # the 20-row graph is captured by the first listen that needs it (launches count at capture) and replayed after
    assert sum(la[:2]) > 0 and sum(la[:2]) % want == 0, la
    assert la[2] == 0 and la2[1:] == [0, 0], (la, la2)   # replays issue nothing
    assert lb == [0, 0, 0]
    np.testing.assert_allclose(pa, pb, atol=5e-4, rtol=0)
    _close(ra, rb, "listen decision rows")
    assert np.array_equal(pa, pa2) and torch.equal(ra, ra2)   # equal state in, equal bits out
    # mlp_weights="mxfp6" alone: no row-stream launch at 20 rows
    C = FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="mxfp6")
    assert C.mlp_mxfp6_rows == 16 and C.llm.stack.mlp_rows == 16 and C.llm.stack.mlp_weights == "mxfp6"
    assert all(L.gu.rows_rb == () and L.down.rows_rb == () for L in C.llm.stack.layers)
    hc, nc = _prefill(C, ids)
    assert nc == 0 and torch.equal(hc, hb)


def test_option_errors(dev):
    from fo.engine import FreezeOmniEngine
    path = os.path.join(ROOT, "configs", "tiny")
    with pytest.raises(ValueError):
        FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="mxfp6", mlp_mxfp6_rows=32)
    with pytest.raises(ValueError):
        FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="bf16", mlp_mxfp6_rows=64)
    with pytest.raises(ValueError):
        FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="fp8", mlp_mxfp6_rows=64)
    with pytest.raises(ValueError):
        FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="mxfp6", mlp_fp8_rows=64)
    with pytest.raises(ValueError):
        FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="mxfp6", mlp_mxfp4_rows=64)


def test_receive_only_replica_streams_the_same_bits(dev):
    from fo.engine import FreezeOmniEngine
    from fo.replica import copy_frozen
    path = os.path.join(ROOT, "configs", "tiny")
    A = FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="mxfp6", mlp_mxfp6_rows=64)
    C = FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="mxfp6", mlp_mxfp6_rows=64,
                         receive_weights=True)
    assert copy_frozen(A, C) > A.llm.mlp_fp6_bytes
    ids = list(range(3, 27))
    outs = []
    for eng in (A, C):
        _force_if_policy_is_empty(eng.llm.stack)
        h, n = _prefill(eng, ids)
        assert n == _per_forward(eng.llm.stack, 24) > 0
        outs.append(h)
    assert torch.equal(outs[0], outs[1])
