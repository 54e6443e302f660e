"""The whole 28-layer Qwen2 forward, eager, with the MLP weights as bf16 and as FP8 under several mlp_fp8_rows, in one
process: a bf16 LLMEngine on the dequantised weights and an FP8 one whose stream_rows / rows_rb are switched per arm.
 * --band 64 (default): the duplex tick shapes (8 sessions x 4 framing-B tokens and 8 x 6, on a few hundred keys per
   session) under bf16, fp8 with mlp_fp8_rows = 16 and fp8 with mlp_fp8_rows = 64; the gemm_w8_rows launches of one
   forward are printed.
 * --band 128: the grouped listen's shape (64 session-chunks x 2 tokens = 128 rows, on about 200 keys each) under bf16,
   fp8 with mlp_fp8_rows = 64 (at this size the same launches as bf16), fp8 with mlp_fp8_rows = 128 under the committed
   ops.W8_ROWS_POLICY, and fp8 with mlp_fp8_rows = 128 and every (GEMM, row blocks) pair forced onto the FP8 stream;
   the gemm_w8_rows128 / gemm_rows launches of one forward are printed.
Each arm owns its sessions with the same context, the arms are alternated, three repeats each; wall time per forward
with one synchronisation after the timed forwards.
python scripts/mlp_fp8_rows_stage.py [--band 64|128] [forwards per repeat] (GPU only)"""
import argparse
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

ap = argparse.ArgumentParser()
ap.add_argument("--band", type=int, choices=(64, 128), default=64)
ap.add_argument("forwards", type=int, nargs="?")
args = ap.parse_args()
BAND = args.band
# sessions, tokens per session and forward, context per session, KV tokens (fp8, bf16 engine), forwards per repeat,
# the launch kinds counted, and the arms: name -> (engine, mlp_fp8_rows, every pair forced onto the stream)
S, NS, CTX, KV, N, KINDS = {64: (8, (4, 6), 320, (32768, 16384), 20, ("gemm_w8_rows",)),
                            128: (64, (2,), 192, (65536, 32768), 10, ("gemm_w8_rows128", "gemm_rows"))}[BAND]
N = args.forwards or N
dev = torch.device("cuda:0")
cfg = configs.get("real")
src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
A = LLMEngine(src, cfg["llm"], dev, kv_tokens=KV[0], mlp_weights="fp8", mlp_rows=BAND)
B = LLMEngine(FakeQuantSource(src), cfg["llm"], dev, kv_tokens=KV[1])
rng = np.random.default_rng(0)
POLICY = {"gu": A.stack.layers[0].gu.rows_rb, "down": A.stack.layers[0].down.rows_rb}


def set_rows(eng, rows, forced):
    for L in eng.stack.layers:
        L.gu.stream_rows = L.down.stream_rows = rows
        L.gu.rows_rb = tuple(range(2, 9)) if forced else POLICY["gu"]
        L.down.rows_rb = tuple(range(2, 9)) if forced else POLICY["down"]
    eng.stack.mlp_rows = rows


arms = {64: {"bf16": (B, None, False), "fp8 rows=16": (A, 16, False), "fp8 rows=64": (A, 64, False)},
        128: {"bf16": (B, None, False), "fp8 rows=64": (A, 64, False), "fp8 rows=128 policy": (A, 128, False),
              "fp8 rows=128 forced": (A, 128, True)}}[BAND]
kvs = {}
for name, (eng, rows, forced) in arms.items():
    if rows is not None:
        set_rows(eng, 16, False)   # the context through the image in every arm
    kvs[name] = [eng.new_seq() for _ in range(S)]
    for s0 in range(0, S, 8):     # the context, 8 sessions x 64 rows per forward
        for c in range(CTX // 64):
            ids = rng.integers(0, eng.V, 8 * 64).tolist()
            eng.forward(eng.embed(ids, round_fp16=True), [(kv, 64) for kv in kvs[name][s0:s0 + 8]])
if BAND == 128:
    print(f"committed ops.W8_ROWS_POLICY: {ops.W8_ROWS_POLICY}", flush=True)
for n in NS:
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
            launches[name] = " / ".join(str(c[k]) for k in KINDS)
            eng.forward(xs[1], [(kv, n) for kv in kvs[name]])
            torch.cuda.synchronize()
            t = time.perf_counter()
            for x in xs[2:]:
                eng.forward(x, [(kv, n) for kv in kvs[name]])
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t) / N * 1e3)
    keys = kvs["bf16"][0].length
    for name in arms:
        print(f"Qwen2 forward {S} x {n} = {S * n} rows, ~{keys} keys, eager, {N} forwards x 3: "
              f"{name:{12 if BAND == 64 else 20}s} "
              f"{'/'.join(f'{t:.3f}' for t in res[name])} ms wall per forward (min {min(res[name]):.3f}), "
              f"{' / '.join(KINDS)} launches per forward {launches[name]}", flush=True)
