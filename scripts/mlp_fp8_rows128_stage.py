"""The whole 28-layer Qwen2 forward, eager, at the grouped listen's shape (64 session-chunks x 2 tokens = 128 rows, on
about 200 keys each) under mlp_weights = bf16, fp8 with mlp_fp8_rows = 64 (at this size the same launches as bf16),
fp8 with mlp_fp8_rows = 128 under the committed ops.W8_ROWS_POLICY, and fp8 with mlp_fp8_rows = 128 and every
(GEMM, row blocks) pair forced onto the FP8 stream (rows_rb): a bf16 LLMEngine on the dequantised weights and an FP8
one whose stream_rows / rows_rb are switched per arm.  Each arm owns 64 sessions with the same context, the arms are
alternated, three repeats each; wall time per forward with one synchronisation after the timed forwards, and the
gemm_w8_rows128 / gemm_rows launches of one forward.
python scripts/mlp_fp8_rows128_stage.py [forwards per repeat] (GPU only)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "freeze-omni_amd"))
from fo import ops  # noqa: E402
from fo.llm import LLMEngine  # noqa: E402
from fo.weights import FakeQuantSource, SynthSource  # noqa: E402
from oracle import configs  # noqa: E402
from oracle.params import all_shapes  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dev = torch.device("cuda:0")
cfg = configs.get("real")
src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
A = LLMEngine(src, cfg["llm"], dev, kv_tokens=65536, mlp_w8=True, mlp_w8_rows=128)
B = LLMEngine(FakeQuantSource(src), cfg["llm"], dev, kv_tokens=32768)
S, n, CTX = 64, 2, 192
rng = np.random.default_rng(0)
POLICY = {"gu": A.stack.layers[0].gu.rows_rb, "down": A.stack.layers[0].down.rows_rb}


def set_rows(eng, rows, forced):
    for L in eng.stack.layers:
        L.gu.stream_rows = L.down.stream_rows = rows
        L.gu.rows_rb = tuple(range(2, 9)) if forced else POLICY["gu"]
        L.down.rows_rb = tuple(range(2, 9)) if forced else POLICY["down"]
    eng.stack.mlp_w8_rows = rows


arms = {"bf16": (B, None, False), "fp8 rows=64": (A, 64, False), "fp8 rows=128 policy": (A, 128, False),
        "fp8 rows=128 forced": (A, 128, True)}
kvs = {}
for name, (eng, rows, forced) in arms.items():
    if rows is not None:
        set_rows(eng, 16, False)   # the context through the image in every arm
    kvs[name] = [eng.new_seq() for _ in range(S)]
    for s0 in range(0, S, 8):     # the context, 8 sessions x 64 rows per forward
        for c in range(CTX // 64):
            ids = rng.integers(0, eng.V, 8 * 64).tolist()
            eng.forward(eng.embed(ids, round_fp16=True), [(kv, 64) for kv in kvs[name][s0:s0 + 8]])
res = {k: [] for k in arms}
launches = {}
for rep in range(3):
    for name, (eng, rows, forced) in arms.items():
        if rows is not None:
            set_rows(eng, rows, forced)
        xs = [eng.embed(rng.integers(0, eng.V, S * n).tolist(), round_fp16=True) for _ in range(N + 2)]
        ops.launch_counts_reset()
        eng.forward(xs[0], [(kv, n) for kv in kvs[name]])
        c = ops.launch_counts()
        launches[name] = (c["gemm_w8_rows128"], c["gemm_rows"])
        eng.forward(xs[1], [(kv, n) for kv in kvs[name]])
        torch.cuda.synchronize()
        t = time.perf_counter()
        for x in xs[2:]:
            eng.forward(x, [(kv, n) for kv in kvs[name]])
        torch.cuda.synchronize()
        res[name].append((time.perf_counter() - t) / N * 1e3)
keys = kvs["bf16"][0].length
print(f"committed ops.W8_ROWS_POLICY: {ops.W8_ROWS_POLICY}", flush=True)
for name in arms:
    print(f"Qwen2 forward {S} x {n} = {S * n} rows, ~{keys} keys, eager, {N} forwards x 3: {name:20s} "
          f"{'/'.join(f'{t:.3f}' for t in res[name])} ms wall per forward (min {min(res[name]):.3f}), "
          f"gemm_w8_rows128 / gemm_rows launches per forward {launches[name][0]} / {launches[name][1]}", flush=True)
