"""The whole 28-layer Qwen2 forward, eager, at the duplex tick shapes (8 sessions x 4 framing-B tokens and 8 x 6, on a
few hundred keys per session) under mlp_weights = bf16, fp8 with mlp_fp8_rows = 16 and fp8 with mlp_fp8_rows = 64, in
one process: a bf16 LLMEngine on the dequantised weights and an FP8 one whose stream_rows is switched per arm.  Each
arm owns 8 sessions with the same context, the arms are alternated, three repeats each; wall time per forward with one
synchronisation after the timed forwards, and the gemm_w8_rows launches of one forward.
python scripts/mlp_fp8_rows_stage.py [forwards per repeat] (GPU only)"""
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda:0")
cfg = configs.get("real")
src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
A = LLMEngine(src, cfg["llm"], dev, kv_tokens=32768, mlp_w8=True, mlp_w8_rows=64)
B = LLMEngine(FakeQuantSource(src), cfg["llm"], dev, kv_tokens=16384)
S, CTX = 8, 320
rng = np.random.default_rng(0)


def set_rows(eng, rows):
    for L in eng.stack.layers:
        L.gu.stream_rows = L.down.stream_rows = rows
    eng.stack.mlp_w8_rows = rows


arms = {"bf16": (B, None), "fp8 rows=16": (A, 16), "fp8 rows=64": (A, 64)}
kvs = {}
for name, (eng, rows) in arms.items():
    kvs[name] = [eng.new_seq() for _ in range(S)]
    for c in range(CTX // 64):   # the context, 8 x 64 rows per forward (the image in every arm)
        ids = rng.integers(0, eng.V, S * 64).tolist()
        eng.forward(eng.embed(ids, round_fp16=True), [(kv, 64) for kv in kvs[name]])
for n in (4, 6):
    res = {k: [] for k in arms}
    launches = {}
    for rep in range(3):
        for name, (eng, rows) in arms.items():
            if rows is not None:
                set_rows(eng, rows)
            xs = [eng.embed(rng.integers(0, eng.V, S * n).tolist(), round_fp16=True) for _ in range(N + 2)]
            ops.launch_counts_reset()
            eng.forward(xs[0], [(kv, n) for kv in kvs[name]])
            launches[name] = ops.launch_counts()["gemm_w8_rows"]
            eng.forward(xs[1], [(kv, n) for kv in kvs[name]])
            torch.cuda.synchronize()
            t = time.perf_counter()
            for x in xs[2:]:
                eng.forward(x, [(kv, n) for kv in kvs[name]])
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t) / N * 1e3)
    keys = kvs["bf16"][0].length
    for name in arms:
        print(f"Qwen2 forward 8 x {n} = {S * n} rows, ~{keys} keys, eager, {N} forwards x 3: {name:12s} "
              f"{'/'.join(f'{t:.3f}' for t in res[name])} ms wall per forward (min {min(res[name]):.3f}), "
              f"gemm_w8_rows launches per forward {launches[name]}", flush=True)
