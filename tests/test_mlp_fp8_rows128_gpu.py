"""mlp_fp8_rows=128 through the engines: Qwen2 steps of 65..128 rows stream the FP8 codes (fo_gemm_w8_rows128) for the
GEMMs and row counts of ops.W8_ROWS_POLICY.  The model does not change: a bf16 engine on the same (dequantised) weights
agrees to the accumulation-order difference between kernels, and the numpy oracle on the same model holds the engine to
the full-depth bounds.  Steps of <= 64 rows dispatch exactly as under mlp_fp8_rows=64."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _close(a, b, what):
    a, b = (t.detach().float().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (a, b))
    np.testing.assert_allclose(a, b, atol=1e-3, rtol=1e-3, err_msg=what)


def _count(kind="gemm_w8_rows128"):
    from fo import ops
    return ops.launch_counts()[kind]


def _per_forward(stack, T, lo=65, hi=128):
    """FP8 launches of the lo..hi-row kernel in one T-row forward under the policy in force (PackedLinearW8.streams)."""
    if not lo <= T <= hi:
        return 0
    return sum(int(L.gu.streams(T)) + int(L.down.streams(T)) for L in stack.layers)


def _force_if_policy_is_empty(stack):
    """Were every (GEMM, row blocks) pair of 5..8 left on the image, the kernel would still be covered: rows_rb is the
    PackedLinearW8 attribute that sends every 17..128-row call to the FP8 kernels."""
    from fo import ops
    if not any(rb >= 5 for v in ops.W8_ROWS_POLICY.values() for rb in v):
        for L in stack.layers:
            L.gu.rows_rb = L.down.rows_rb = tuple(range(2, 9))


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


def test_real_geometry_listen_shapes_against_bf16_engine_and_oracle(dev):
    """Eight sessions; steps of 8 x 9, 12 and 16 tokens (72, 96, 128 rows: a duplex tick that starts a turn, and the
    grouped listen), then 8 x 4 (the 17..64-row kernels) and 8 x 1 (the <= 16-row ones).  C, with mlp_rows=64, runs
    the same steps without a 65..128-row FP8 launch: its 72-row step (no FP8 history yet) has the bf16 engine's bits."""
    from fo import ops
    from fo.llm import LLMEngine
    from fo.weights import FakeQuantSource, SynthSource
    from oracle import configs, nets
    from oracle.params import all_shapes
    cfg = configs.get("real")
    cfg["llm"]["num_hidden_layers"] = 2
    src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
    A = LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16, mlp_weights="fp8", mlp_rows=128)
    model = FakeQuantSource(src)
    B = LLMEngine(model, cfg["llm"], dev, kv_tokens=4096, page_size=16)
    C = LLMEngine(src, cfg["llm"], dev, kv_tokens=4096, page_size=16, mlp_weights="fp8", mlp_rows=64)
    _force_if_policy_is_empty(A.stack)
    assert A.weight_bytes == B.weight_bytes and A.stack.mlp_rows == 128 and A.stack.mlp_weights == "fp8"
    S = 8
    per = [9, 12, 16, 4, 1]
    rng = np.random.default_rng(8)
    steps = [rng.integers(0, A.V, S * n).tolist() for n in per]
    got = {}
    for name, eng in (("A", A), ("B", B), ("C", C)):
        kvs = [eng.new_seq() for _ in range(S)]
        hs, lgs, xs = [], [], []
        try:
            for n, ids in zip(per, steps):
                x = eng.embed(ids, round_fp16=True)
                xs.append(x[:n].cpu().numpy())   # session 0's rows come first
                ops.launch_counts_reset()
                h, bm = eng.forward(x, [(kv, n) for kv in kvs])
                c = ops.launch_counts()
                T = S * n
                if name == "B":
                    want = (0, 0, 0, 0)
                elif T <= 16:
                    want = (0, 0, 2, 2)
                else:
                    want = (_per_forward(eng.stack, T) if name == "A" else 0, _per_forward(eng.stack, T, 17, 64), 0, 0)
                    assert name == "C" or want[0] > 0 or T <= 64
                    assert T > 64 or want[1] > 0 or not any(ops.W8_ROWS_POLICY.values())
                assert (c["gemm_w8_rows128"], c["gemm_w8_rows"], c["gemm_w8"], c["gemm_w8_xs"]) == want, (name, T, c)
                hs.append(h.clone())
                lgs.append(eng.logits(h, bm.last_rows_host).clone())
        finally:
            for kv in kvs:
                kv.free()
        got[name] = (hs, lgs, xs)
    for s, n in enumerate(per):
        _close(got["A"][0][s], got["B"][0][s], f"{S} x {n} rows: hidden rows, FP8 against the bf16 engine")
        _close(got["A"][1][s], got["B"][1][s], f"{S} x {n} rows: logits, FP8 against the bf16 engine")
    assert torch.equal(got["C"][0][0], got["B"][0][0])   # 72 rows under mlp_rows=64: the same kernels, same image
    # the oracle on the same model, session 0
    W = _DeviceWeights(model)
    q = nets.Qwen2(W, cfg)
    okv = nets.KV(2)
    for s, n in enumerate(per):
        h = q.forward(got["A"][2][s], okv)
        hv = got["A"][0][s][n - 1].float().cpu().numpy()
        dh = float(np.abs(hv - h[-1]).max())
        rel = float(np.linalg.norm(hv - h[-1]) / np.linalg.norm(h[-1]))
        assert dh < 1e-2 and rel < 2e-3, (s, dh, rel)
        np.testing.assert_allclose(got["A"][1][s][0].float().cpu().numpy(), q.logits(h[-1:])[0], atol=5e-3, rtol=5e-3,
                                   err_msg=f"{S} x {n} rows: logits against the oracle")


# ------------------------------------------------------------------ tiny config, the whole engine
def _group_flow(eng, feats, n_sess, n_chunks, C):
    """System prompt, chunk 0 after apply_chat_prefix, then every chunk through listen_pipe(C) (the benchmark's order).
    Returns (state probabilities, decision rows, gemm_w8_rows128 launches of the whole flow)."""
    base = eng.system_role("<|im_start|>system\nYou are a helpful assistant.")
    kvs = [base.fork() for _ in range(n_sess)]
    state = [dict(enc_cache=None, ada_cache=None, pe_index=0) for _ in range(n_sess)]
    probs, rows = [], []

    def record(groups):
        for res in groups or []:
            probs.append([(r["probs"]["state_1"], r["probs"]["state_2"]) for r in res])
            rows.append(torch.stack([r["hidden_row"][0][r["hidden_row"][1]].clone() for r in res]))

    before = _count()
    try:
        pipe = eng.listen_pipe(C)
        for c in range(n_chunks):
            items = [dict(identity="user", status="ipu_sl" if c == 0 else "ipu_cl", feats=feats[(c + 4 * u) % 13],
                          kv=kvs[u], **state[u]) for u in range(n_sess)]
            if c == 0:
                items = eng.apply_chat_prefix(items)
                for u, it in enumerate(items):
                    state[u] = dict(enc_cache=it["enc_cache"], ada_cache=it["ada_cache"], pe_index=it["pe_index"])
            pe_next, prev = pipe.push(items)
            for u in range(n_sess):
                state[u]["pe_index"] = pe_next[u]
            record(prev)
        record(pipe.flush())
    finally:
        for kv in kvs + [base]:
            kv.free()
    assert len(probs) == n_chunks
    return np.asarray(probs), torch.stack(rows), _count() - before


def test_tiny_engine_grouped_listen_streams_128_and_112_rows(dev):
    from fo.engine import FreezeOmniEngine
    path = os.path.join(ROOT, "configs", "tiny")
    A = FreezeOmniEngine(path, device=dev, max_sessions=12, mlp_weights="fp8", mlp_fp8_rows=128)
    assert A.mlp_fp8_rows == 128 and A.llm.stack.mlp_rows == 128 and A.llm.stack.mlp_weights == "fp8"
    B = FreezeOmniEngine(path, device=dev, max_sessions=12, source=A.src)
    assert B.mlp_fp8_rows == 16
    _force_if_policy_is_empty(A.llm.stack)
    feats = torch.from_numpy(np.load(os.path.join(G, "fbank.npz"))["A_feats"]).to(dev)   # [13, 19, 80]
    # 8 sessions x 23 chunks in groups of 8: two full groups (one capture per slot) and a 7-chunk partial group
    pa, ra, la = _group_flow(A, feats, 8, 23, 8)
    g = next(v for k, v in A._lgraphs.items() if k[3:4] == ("group",))
    assert g.n == 128 and g.n1 == 16
    stack = A.llm.stack
    assert la == 2 * _per_forward(stack, 128) + _per_forward(stack, 112) and la > 0, la   # counted at capture
    pa2, ra2, la2 = _group_flow(A, feats, 8, 23, 8)
    assert la2 == 0                                                # replays issue nothing
    assert np.array_equal(pa, pa2) and torch.equal(ra, ra2)       # equal state in, equal bits out
    pb, rb, lb = _group_flow(B, feats, 8, 23, 8)
    assert lb == 0
    np.testing.assert_allclose(pa, pb, atol=5e-4, rtol=0)
    _close(ra, rb, "grouped listen decision rows")


def test_option_errors(dev):
    from fo.engine import FreezeOmniEngine
    path = os.path.join(ROOT, "configs", "tiny")
    with pytest.raises(ValueError):
        FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="bf16", mlp_fp8_rows=128)


def test_receive_only_replica_streams_the_same_bits(dev):
    from fo.engine import FreezeOmniEngine
    from fo.replica import copy_frozen
    path = os.path.join(ROOT, "configs", "tiny")
    A = FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="fp8", mlp_fp8_rows=128)
    C = FreezeOmniEngine(path, device=dev, max_sessions=2, mlp_weights="fp8", mlp_fp8_rows=128, receive_weights=True)
    assert copy_frozen(A, C) > A.llm.mlp_fp8_bytes
    ids = [3 + (7 * i) % 24 for i in range(100)]
    outs = []
    for eng in (A, C):
        _force_if_policy_is_empty(eng.llm.stack)
        kv = eng.llm.new_seq()
        try:
            before = _count()
            h, _ = eng.llm.forward(eng.llm.embed(ids, round_fp16=True), [(kv, len(ids))])
            assert _count() - before == _per_forward(eng.llm.stack, 100) > 0
            outs.append(h.clone())
        finally:
            kv.free()
    assert torch.equal(outs[0], outs[1])
