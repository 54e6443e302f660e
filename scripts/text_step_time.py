"""Wall and device time of one text-decode step (TextGraph: 28 Qwen2 layers + lm_head + sampler) for B
sessions at real geometry after a ~150-token context, as the bench's speak stage runs it.
python scripts/text_step_time.py [B] [steps] [fp8|mxfp4|mxfp6|a,b,..] [head] [attn] [force] (GPU only; run under rocprofv3 --kernel-trace
--stats for the per-kernel split).  The third argument `fp8` turns mlp_weights="fp8" on (the MLP streams FP8 codes);
`mxfp4` times the bf16, fp8 and mxfp4 engines one after the other in the same call, so the three lines share a process
and a clock; a comma-separated list (`bf16,mxfp4`; `mxfp4,` for that
engine alone) times exactly those.  The optional fourth argument is
lm_head_weights (`bf16`, `fp8`, `mxfp4`, `mxfp6`, `all`: the three older heads under every MLP mode of the call, or
`same`: each MLP mode under the head of its own format), the optional
fifth attn_weights in the same forms (`all`: the three under every MLP mode and head of the call); a sixth argument
`force` puts q|k|v and o on their code streams whatever ops.ATTN_POLICY says (A/B only).  The GB figure
counts the bytes the step actually streams: codes where a GEMM streams them, its bf16 image where it does not."""
import gc
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "freeze-omni_amd"))
from fo.engine import FreezeOmniEngine  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
N = int(sys.argv[2]) if len(sys.argv) > 2 else 40
MODE = sys.argv[3] if len(sys.argv) > 3 else "bf16"
HEAD = sys.argv[4] if len(sys.argv) > 4 else "bf16"
ATTN = sys.argv[5] if len(sys.argv) > 5 else "bf16"
FORCE = len(sys.argv) > 6 and sys.argv[6] == "force"
dev = torch.device("cuda:0")


def run(mode, head="bf16", attn="bf16"):
    eng = FreezeOmniEngine(os.path.join(ROOT, "configs", "real"), device=dev, max_sessions=max(8, B), mlp_weights=mode,
                           lm_head_weights=head, attn_weights=attn)
    if FORCE and attn != "bf16":
        for l in eng.llm.stack.layers:
            l.qkv.stream = l.o.stream = True
    base = eng.system_role("<|im_start|>system\nYou are a helpful assistant.")
    kvs = [base.fork() for _ in range(B)]
    ctx = list(range(100, 230))
    eng.text_step([(kv, ctx) for kv in kvs])          # ~150-token context per session
    ids, _ = eng.text_step([(kv, [1]) for kv in kvs])
    for _ in range(5):
        ids, _ = eng.text_step([(kv, [i]) for kv, i in zip(kvs, ids)])
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(N):
        ids, _ = eng.text_step([(kv, [i]) for kv, i in zip(kvs, ids)])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t) / N
    gb = (eng.llm.stack.weight_bytes + eng.llm.lm_head.nbytes) / 1e9
    L = eng.llm.stack.layers
    if mode == "fp8":   # the MLP streams its codes instead of its bf16 image
        gb += (eng.llm.mlp_fp8_bytes - sum(l.gu.nbytes + l.down.nbytes for l in L)) / 1e9
    if mode == "mxfp4":   # ... the GEMMs of ops.W4_POLICY do
        gb += sum(lin.fp4_nbytes - lin.nbytes for l in L for lin in (l.gu, l.down) if lin.streams(B)) / 1e9
    if mode == "mxfp6":   # ... the GEMMs of ops.W6_POLICY do
        gb += sum(lin.fp6_nbytes - lin.nbytes for l in L for lin in (l.gu, l.down) if lin.streams(B)) / 1e9
    lh = eng.llm.lm_head
    if head != "bf16" and lh.streams(B):   # the head streams its codes instead of its bf16 image
        gb += (getattr(lh, {"fp8": "fp8_nbytes", "mxfp4": "fp4_nbytes", "mxfp6": "fp6_nbytes"}[head]) - lh.nbytes) / 1e9
    if attn != "bf16":   # q|k|v and o stream their codes where ops.ATTN_POLICY (or `force`) says so
        gb += sum((lin.fp8_nbytes if attn == "fp8" else lin.fp4_nbytes) - lin.nbytes
                  for l in L for lin in (l.qkv, l.o) if lin.streams(B)) / 1e9
    tag = mode if head == "bf16" else f"{mode} lm_head_weights={head}"
    if ATTN != "bf16":
        tag += f" attn_weights={attn}{' (forced)' if FORCE and attn != 'bf16' else ''}"
    print(f"text step B={B} mlp_weights={tag}: {dt * 1e3:.3f} ms wall/step, {gb:.2f} GB weights -> {gb / dt / 1e3:.2f} TB/s "
          f"(roofline {gb / 8.0:.3f} ms at 8 TB/s)", flush=True)


for mode in (("bf16", "fp8", "mxfp4") if MODE == "mxfp4" else tuple(m for m in MODE.split(",") if m)):
    for head in (("bf16", "fp8", "mxfp4") if HEAD == "all" else ((mode,) if HEAD == "same" else (HEAD,))):
        for attn in (("bf16", "fp8", "mxfp4") if ATTN == "all" else (ATTN,)):
            run(mode, head, attn)
            gc.collect()
            torch.cuda.empty_cache()
