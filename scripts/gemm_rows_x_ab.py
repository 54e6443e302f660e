"""A/B of bf16 GEMM inputs for the 65..128-row Qwen2 GEMMs (x_round="bf16" / llm_rows_x="bf16") against
the fp32 arm (bf16 hi / lo split), both on k_gemm_rows + k_gemm_reduce and on the same weights, in one process.
 * --part gemm: the four GEMMs of a Qwen2 layer -- q|k|v (+ bias + RoPE + KV append, RMSNorm consumer), o (+ residual +
   next-norm statistics), gate/up (SwiGLU, RMSNorm consumer), down (+ residual + statistics) -- at 80, 96, 112 and 128
   rows.  Per-launch device time (stream + reduce together) from one replayed hipGraph of launches that walk more than
   512 MB of weight copies in both arms (past the 256 MB Infinity Cache), the arms alternated, --repeats repeats each:
   median and repeat-to-repeat spread (max - min).  The bf16 arm "wins" where the fp32 median exceeds its median by
   more than the fp32 arm's spread.  Each GEMM's armed output is checked bit for bit against the unarmed launch on
   X.bfloat16().float().  Under `rocprofv3 --kernel-trace --stats` (runs of their own, one per row count: --rows M
   --repeats 1 --gemms qkv gu down, and --gemms o, which shares down's instantiation) the kernel table splits the
   stream from its reduce.
 * --part stage: one 28-layer LLMEngine whose stack's rows_x is switched per arm: the eager 128-row forward (64
   session-chunks x 2 tokens on ~192 keys, wall time per forward with one synchronisation) and the captured 8-chunk
   Qwen2 stage (the ListenGraph body at 8 chunks x 8 sessions x 2 tokens: layers, final norm, state head; device time
   per replay), arms alternated.
python scripts/gemm_rows_x_ab.py [--part gemm|stage|all] [--rows M ...] [--repeats R] [--gemms qkv o gu down] (GPU only)"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_graph_sweep_util import graph_time  # noqa: E402
from fo import _lib, ops  # noqa: E402
from fo.ops import PackedLinear  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=("gemm", "stage", "all"), default="all")
ap.add_argument("--rows", type=int, nargs="*", default=[80, 96, 112, 128])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--gemms", nargs="*", default=["qkv", "o", "gu", "down"])
args = ap.parse_args()
dev = torch.device("cuda:0")
D, I, H, KVH, hd = 3584, 18944, 28, 4, 128
g = torch.Generator(device=dev).manual_seed(0)
ARMS = (("fp32", None), ("bf16", "bf16"))
lib = _lib.load()


def rnd(*s, scale=0.02):
    return torch.randn(*s, device=dev, generator=g) * scale


def fmt(v):
    return "/".join(f"{t:.1f}" for t in v)


def report(name, M, res, nbytes, exact, unit="us"):
    med = {a: statistics.median(v) for a, v in res.items()}
    spread = {a: max(v) - min(v) for a, v in res.items()}
    gain = med["fp32"] - med["bf16"]
    verdict = "bf16 WINS" if gain > spread["fp32"] else ("bf16 LOSES" if -gain > spread["fp32"] else "within the spread")
    rate = f" ({nbytes / 1e6:.0f} MB, fp32 {nbytes / med['fp32'] / 1e6:4.2f} TB/s)" if nbytes else ""
    print(f"{name:15s} M={M:3d}  fp32 {fmt(res['fp32'])} {unit} median {med['fp32']:.1f} spread {spread['fp32']:.1f}  "
          f"bf16 {fmt(res['bf16'])} {unit} median {med['bf16']:.1f} spread {spread['bf16']:.1f}{rate}  "
          f"bf16/fp32 {med['bf16'] / med['fp32']:.3f}  {verdict}{exact}", flush=True)


def ab(name, make, ncp, M, nbytes):
    """make(i, x_round) -> a closure launching weight copy i on X; closure(rounded=True / False) launches it once on
    X.bfloat16().float() / on X (restoring the residual first) and returns clones of everything it wrote."""
    res = {a: [] for a, _ in ARMS}
    ops.launch_counts_reset()
    ops.rows_xb_launch_count_reset()
    for _, xr in ARMS:
        make(0, xr)()
    c = ops.launch_counts()
    assert c["gemm_rows"] == 2 and ops.rows_xb_launch_count() == 1, (name, M, c)   # both arms on k_gemm_rows
    for _ in range(args.repeats):
        for arm, xr in ARMS:
            fns = [make(i, xr) for i in range(ncp)]
            it = iter(range(1 << 30))
            res[arm].append(graph_time(lambda: fns[next(it) % ncp](), ncp * max(1, 48 // ncp)))
    a, b = make(0, "bf16")(rounded=False), make(0, None)(rounded=True)
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for p, q in zip(a, b))
    report(name, M, res, nbytes, "  armed(X) == unarmed(bf16(X)): " + ("bit-exact" if same else "DIFFERS"))


def gemm_part():
    specs = {"qkv": 17, "o": 21, "gu": 2, "down": 4}   # copies: each GEMM walks > 512 MB of packed weight
    lins = {}
    if "qkv" in args.gemms:
        lins["qkv"] = [PackedLinear(rnd(H * hd + 2 * KVH * hd, D).to(torch.bfloat16), rnd(H * hd + 2 * KVH * hd),
                                    rope_hd=hd) for _ in range(specs["qkv"])]
    if "o" in args.gemms:
        lins["o"] = [PackedLinear(rnd(D, D).to(torch.bfloat16)) for _ in range(specs["o"])]
    if "gu" in args.gemms:
        lins["gu"] = [PackedLinear(rnd(I, D).to(torch.bfloat16), swiglu_up=rnd(I, D).to(torch.bfloat16))
                      for _ in range(specs["gu"])]
    if "down" in args.gemms:
        lins["down"] = [PackedLinear(rnd(D, I).to(torch.bfloat16)) for _ in range(specs["down"])]
    for k, v in lins.items():
        print(f"{k}: {len(v)} copies x {v[0].nbytes / 1e6:.1f} MB = {len(v) * v[0].nbytes / 1e6:.0f} MB", flush=True)
    cos = torch.rand(4096, hd // 2, device=dev, generator=g)
    sin = torch.rand(4096, hd // 2, device=dev, generator=g)
    PS, pages = 16, 64
    kc = torch.zeros(pages, KVH, PS, hd, device=dev)
    vc = torch.zeros_like(kc)
    gam = torch.rand(D, device=dev, generator=g) + 0.5
    for M in args.rows:
        xd, xi, res0 = rnd(M, D, scale=1.0), rnd(M, I, scale=1.0), rnd(M, D, scale=1.0)
        xdr, xir = xd.bfloat16().float(), xi.bfloat16().float()
        stats = ops.RowStats(128, dev)   # a producer's statistics for the RMSNorm consumers
        PackedLinear(rnd(D, 1024).to(torch.bfloat16))(
            rnd(M, 1024, scale=1.0), out=res0.clone(), residual=True, M=M,
            stats_out=stats.set(torch.ones(D, device=dev), torch.empty(M, D, device=dev)))
        pos = torch.arange(100, 100 + M, dtype=torch.int32, device=dev)
        slot = torch.arange(5, 5 + M, dtype=torch.int32, device=dev)
        qo = torch.empty(M, H * hd, device=dev)
        y = res0.clone()
        yg = torch.empty(M, D, device=dev)
        so = ops.RowStats(128, dev)
        m = torch.empty(M, I, device=dev)

        def mk_qkv(i, xr):
            def f(rounded=None):
                lins["qkv"][i].qkv_rope(xdr if rounded else xd, M, pos, slot, cos, sin, qo, kc, vc, H, KVH, PS,
                                        norm=(stats, 1e-6), x_round=xr)
                return None if rounded is None else [qo.clone(), kc.clone(), vc.clone()]
            return f

        def mk_plain(key, xin, xinr):
            def mk(i, xr):
                def f(rounded=None):
                    if rounded is not None:
                        y.copy_(res0)
                    lins[key][i](xinr if rounded else xin, out=y, residual=True, M=M, stats_out=so.set(gam, yg), x_round=xr)
                    return None if rounded is None else [y.clone(), yg.clone(), so.buf[:M * so.groups].clone()]
                return f
            return mk

        def mk_gu(i, xr):
            def f(rounded=None):
                lins["gu"][i](xdr if rounded else xd, out=m, M=M, norm=(stats, 1e-6), x_round=xr)
                return None if rounded is None else [m.clone()]
            return f

        makers = {"qkv": ("q|k|v+rope", mk_qkv), "o": ("o+res+stats", mk_plain("o", xd, xdr)),
                  "gu": ("gate/up+rms", mk_gu), "down": ("down+res+stats", mk_plain("down", xi, xir))}
        for key in args.gemms:
            name, mk = makers[key]
            ab(name, mk, len(lins[key]), M, lins[key][0].nbytes)


def stage_part():
    from fo.engine import ListenGraph, _HostRing
    from fo.kv import GroupMeta
    from fo.llm import LLMEngine
    from fo.weights import SynthSource
    from oracle import configs
    from oracle.params import all_shapes
    cfg = configs.get("real")
    src = SynthSource(cfg["seed"], all_shapes(cfg), dev, cfg["overrides"])
    llm = LLMEngine(src, cfg["llm"], dev, kv_tokens=65536)
    nl = len(llm.stack.layers)
    rng = np.random.default_rng(0)
    S, n, CTX, N = 64, 2, 192, 10
    # ---- the eager 128-row forward: each arm owns its sessions with the same context
    kvs = {}
    for arm, _ in ARMS:
        kvs[arm] = [llm.new_seq() for _ in range(S)]
        for s0 in range(0, S, 8):
            for _ in range(CTX // 8):   # the context through <= 64-row forwards (no bf16 form in either arm)
                ids = rng.integers(0, llm.V, 8 * 8).tolist()
                llm.forward(llm.embed(ids, round_fp16=True), [(kv, 8) for kv in kvs[arm][s0:s0 + 8]])
    res = {a: [] for a, _ in ARMS}
    took = {}
    for _ in range(args.repeats):
        for arm, _x in ARMS:
            llm.stack.rows_x = arm
            xs = [llm.embed(rng.integers(0, llm.V, S * n).tolist(), round_fp16=True) for _ in range(N + 2)]
            ops.launch_counts_reset()
            ops.rows_xb_launch_count_reset()
            llm.forward(xs[0], [(kv, n) for kv in kvs[arm]])
            took[arm] = (ops.launch_counts()["gemm_rows"], ops.rows_xb_launch_count())
            llm.forward(xs[1], [(kv, n) for kv in kvs[arm]])
            torch.cuda.synchronize()
            t = time.perf_counter()
            for x in xs[2:]:
                llm.forward(x, [(kv, n) for kv in kvs[arm]])
            torch.cuda.synchronize()
            res[arm].append((time.perf_counter() - t) / N * 1e6)
    print(f"eager forward: gemm_rows / bf16-X launches per forward: {took}", flush=True)
    assert took["fp32"] == (4 * nl, 0) and took["bf16"] == (4 * nl, 4 * nl), took
    report(f"eager {nl}-layer", S * n, res, 0, f"  (~{kvs['fp32'][0].length} keys, {N} forwards per repeat, wall)")
    for v in kvs.values():
        for kv in v:
            kv.free()
    # ---- the captured 8-chunk Qwen2 stage (tests/test_real_qwen2_gpu.py's listen-groups harness)
    B, To, C = 8, 2, 8
    n1 = B * To
    seqs = [llm.new_seq() for _ in range(B)]
    for _ in range(4):   # 32 keys of context per session (the stage is timed on its GEMMs: attention is 14 us a layer)
        llm.forward(llm.embed(rng.integers(0, llm.V, 64).tolist(), round_fp16=True), [(q, 8) for q in seqs])
    torch.cuda.synchronize()
    main = ops.engine_stream(dev)
    max_keys = max(max(q.length for q in seqs) + 64 * 2 * C + 1024, 2048)
    gm = GroupMeta(B, To, C, llm.H // llm.KVH, max_keys, llm.pool.PS, dev)
    x = torch.empty(C * n1, llm.D, dtype=torch.float32, device=dev)
    x_in = llm.embed(rng.integers(0, llm.V, C * n1).tolist(), round_fp16=True)
    ws = llm.stack.workspace(C * n1, ops.attn_nsplit(max_keys, C * B, llm.KVH), dev)
    probs = torch.empty(C * B, 3, dtype=torch.float32, device=dev)
    ring = _HostRing(gm.size)
    with torch.cuda.stream(main):
        ops.Runtime.get(dev)

    def body():   # ListenGraph._llm_body at C chunks, after the copy that restores its input
        x.copy_(x_in)
        llm.stack.forward(x, gm.metas[C], ws)
        ops.rmsnorm(x, llm.norm, llm.eps, out=x)
        ops.state_head(x, gm.rows[:C * B], llm.head_w, llm.head_b, probs)

    execs = {}
    for arm, _x in ARMS:
        llm.stack.rows_x = arm
        ops.launch_counts_reset()
        ops.rows_xb_launch_count_reset()
        execs[arm] = ListenGraph._capture(main, body)
        print(f"captured stage, {arm}: gemm_rows {ops.launch_counts()['gemm_rows']}, bf16-X launches "
              f"{ops.rows_xb_launch_count()}", flush=True)
    k, hb = ring.next()
    gm.fill(hb, seqs, C)
    ring.upload(k, gm.buf, main)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    lib.fo_event_create(ctypes.byref(e0))
    lib.fo_event_create(ctypes.byref(e1))
    s = main.cuda_stream
    res = {a: [] for a, _ in ARMS}
    reps = 20
    for _ in range(args.repeats):
        for arm, _x in ARMS:
            _lib.call("fo_graph_launch", execs[arm], s)
            main.synchronize()
            lib.fo_event_record(e0, s)
            for _ in range(reps):
                _lib.call("fo_graph_launch", execs[arm], s)
            lib.fo_event_record(e1, s)
            main.synchronize()
            ms = ctypes.c_float()
            lib.fo_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            res[arm].append(ms.value / reps * 1e3)
    report(f"captured C={C}", C * n1, res, 0, f"  ({nl} layers + norm + state head, ~{seqs[0].length} keys, {reps} replays "
           f"per repeat, device time)")
    torch.cuda.synchronize()
    for ex in execs.values():
        _lib.call("fo_graph_destroy", ex)
    ring.destroy()
    for q in seqs:
        q.free()


if args.part in ("gemm", "all"):
    gemm_part()
if args.part in ("stage", "all"):
    stage_part()
