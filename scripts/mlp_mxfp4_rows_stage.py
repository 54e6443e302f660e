"""The whole 28-layer Qwen2 forward, eager, with the MLP weights as bf16 and as MXFP4 under mlp_mxfp4_rows = 16 and 64,
in one process (scripts/mlp_fp8_rows_stage.py's method on the MXFP4 option): a bf16 LLMEngine on the dequantised
weights and an MXFP4 one whose stream_rows / rows_rb are switched per arm.  The duplex tick shapes (8 sessions x 4
framing-B tokens and 8 x 6, on a few hundred keys per session) under bf16, mxfp4 with rows = 16, mxfp4 with rows = 64
under the committed ops.W4_ROWS_POLICY and, for the record of what the policy decides about, mxfp4 with rows = 64 and
every (GEMM, row blocks) pair forced onto the row stream; the fo_gemm_w4_rows calls of one forward are printed.
--fmt mxfp6 runs the same arms on the MXFP6 option (mlp_mxfp6_rows, ops.W6_ROWS_POLICY, fo_gemm_w6_rows).
Each arm owns its sessions with the same context, the arms are alternated, three repeats each; wall time per forward
with one synchronisation after the timed forwards.
python scripts/mlp_mxfp4_rows_stage.py [--fmt mxfp4|mxfp6] [forwards per repeat] (GPU only)"""
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

S, NS, CTX, KV = 8, (4, 6), 320, (32768, 16384)
ap = argparse.ArgumentParser()
ap.add_argument("--fmt", choices=("mxfp4", "mxfp6"), default="mxfp4", help="the MLP format under test")
ap.add_argument("forwards", nargs="?", type=int, default=20)
args = ap.parse_args()
FMT, N = args.fmt, args.forwards
POLICY_NAME, ENTRY, rows_count, counts_reset = {
    "mxfp4": ("W4_ROWS_POLICY", "fo_gemm_w4_rows", ops.w4_rows_launch_count, ops.w4_launch_counts_reset),
    "mxfp6": ("W6_ROWS_POLICY", "fo_gemm_w6_rows", ops.w6_rows_launch_count, ops.w6_launch_counts_reset)}[FMT]
dev = torch.device("cuda:0")
cfg = configs.get("real")
src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
A = LLMEngine(src, cfg["llm"], dev, kv_tokens=KV[0], mlp_weights=FMT, mlp_rows=64)
B = LLMEngine(FakeQuantSource(src, FMT), cfg["llm"], dev, kv_tokens=KV[1])
rng = np.random.default_rng(0)
POLICY = {"gu": A.stack.layers[0].gu.rows_rb, "down": A.stack.layers[0].down.rows_rb}


def set_rows(eng, rows, forced):
    for L in eng.stack.layers:
        L.gu.stream_rows = L.down.stream_rows = rows
        L.gu.rows_rb = (2, 3, 4) if forced else POLICY["gu"]
        L.down.rows_rb = (2, 3, 4) if forced else POLICY["down"]
    eng.stack.mlp_rows = rows


# name -> (engine, mlp_<format>_rows, every pair forced onto the row stream)
arms = {"bf16": (B, None, False), f"{FMT} rows=16": (A, 16, False), f"{FMT} rows=64 policy": (A, 64, False),
        f"{FMT} rows=64 forced": (A, 64, True)}
kvs = {}
for name, (eng, rows, forced) in arms.items():
    if rows is not None:
        set_rows(eng, 16, False)   # the context through the image in every arm
    kvs[name] = [eng.new_seq() for _ in range(S)]
    for c in range(CTX // 64):     # the context, 8 sessions x 64 rows per forward
        ids = rng.integers(0, eng.V, 8 * 64).tolist()
        eng.forward(eng.embed(ids, round_fp16=True), [(kv, 64) for kv in kvs[name]])
print(f"committed ops.{POLICY_NAME}: {getattr(ops, POLICY_NAME)}", flush=True)
for n in NS:
    res = {k: [] for k in arms}
    launches = {}
    for rep in range(3):
        for name, (eng, rows, forced) in arms.items():
            if rows is not None:
                set_rows(eng, rows, forced)
            xs = [eng.embed(rng.integers(0, eng.V, S * n).tolist(), round_fp16=True) for _ in range(N + 2)]
            counts_reset()
            eng.forward(xs[0], [(kv, n) for kv in kvs[name]])
            launches[name] = rows_count()
            eng.forward(xs[1], [(kv, n) for kv in kvs[name]])
            torch.cuda.synchronize()
            t = time.perf_counter()
            for x in xs[2:]:
                eng.forward(x, [(kv, n) for kv in kvs[name]])
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t) / N * 1e3)
    keys = kvs["bf16"][0].length
    for name in arms:
        print(f"Qwen2 forward {S} x {n} = {S * n} rows, ~{keys} keys, eager, {N} forwards x 3: {name:20s} "
              f"{'/'.join(f'{t:.3f}' for t in res[name])} ms wall per forward (min {min(res[name]):.3f}, median "
              f"{sorted(res[name])[1]:.3f}), {ENTRY} calls per forward {launches[name]}", flush=True)
