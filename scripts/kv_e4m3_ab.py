"""The FP8 paged-KV layout (llm_kv="e4m3") against the fp32 and bf16 ones on the Qwen2 shapes (28 q / 4 kv
heads of 128, pages of 16): the three pools in one process holding the same values (e4m3 codes x 2^e, which are bf16
values), the arms alternated, every figure the per-launch device time of 50 launches captured as one hipGraph and
replayed, three repeats per arm (best of three, the repeats and their spread beside it).

fo_attention on DESIGN §5.6's seven shapes
  the text step       8 x 1 token  at 150, 448, 1,000 and 4,000 keys (the TextGraph's launch: tickets, 128-key splits)
  the listen chunk    8 x 2 tokens at 200 keys (the ListenGraph's launch)
  the duplex tick     8 x 4 tokens at 600 keys (the eager launch: 16 items of 2 tokens, keys per split sized per launch)
  the 8-chunk group   64 items x 2 tokens at 200 keys
and the q|k|v projection + RoPE + append (K = 3584, synthetic weights) at 8, 16, 32 and 128 rows (16 and 32 rows on
packed X): for the FP8 pool the projection into the staging cache plus fo_kv8_append, with the append launch's own time
listed separately.

A replayed launch re-reads the same K / V, so what it reads sits in the L2 / Infinity Cache as far as it fits there, in
every arm.  Each attention row also reports whether the three arms' outputs are equal (they must be).

python scripts/kv_e4m3_ab.py            the two tables above (profiles/kv_e4m3_layout_ab.txt)
python scripts/kv_e4m3_ab.py text       the B = 8 text step (TextGraph, 28 layers at real geometry, wall time per step)
                                        at 150 and at 4,000 keys, one engine per pool (profiles/kv_e4m3_text_step.txt)
GPU only."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "freeze-omni_amd"))
from gemm_graph_sweep_util import graph_time  # noqa: E402
from fo import _lib, ops, tables  # noqa: E402
from fo.kv import BatchMeta, KVPool, KVSeq  # noqa: E402
from fo.quant import quantize_kv_rows  # noqa: E402

dev = torch.device("cuda:0")
H, KVH, hd, PS, D = 28, 4, 128, 16, 3584
REPS, REPEATS = 50, 3
ARMS = ("fp32", "bf16", "e4m3")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn}
g = torch.Generator(device=dev).manual_seed(0)
print(f"library {_lib.LIB_PATH}", flush=True)


def arms(fns):
    """Three repeats of each arm, alternated; -> {arm: times in us}."""
    t = {a: [] for a in fns}
    for _ in range(REPEATS):
        for a, f in fns.items():
            t[a].append(graph_time(f, REPS))
    return t


def row(name, t, extra=""):
    best = {a: min(v) for a, v in t.items()}
    cols = "   ".join(f"{a} {best[a]:7.2f} us ({' '.join(f'{x:.2f}' for x in v)}; spread {max(v) - best[a]:.2f})"
                      for a, v in t.items())
    ratios = ""
    if "e4m3" in best and "bf16" in best:
        ratios = f"   e4m3 / bf16 {best['e4m3'] / best['bf16']:.3f}  e4m3 / fp32 {best['e4m3'] / best['fp32']:.3f}"
    print(f"{name:44s} {cols}{ratios} {extra}", flush=True)
    return best


def pools(n_pages):
    return {a: KVPool(1, KVH, hd, n_pages, PS, dev, dtype=DTYPES[a]) for a in ARMS}


def scales_of(pool):
    return dict(kscale=pool.ks[0], vscale=pool.vs[0]) if pool.fp8 else {}


# ------------------------------------------------------------------ fo_attention
def attention(name, n_seq, tokens, L, graph):
    n_pages = n_seq * ((L + PS - 1) // PS) + 1
    p = pools(n_pages)
    for nm in ("k", "v"):   # random rows through the CPU model: codes and scales, and their bf16 image in the other pools
        q, e, img = quantize_kv_rows(torch.randn(n_pages, KVH, PS, hd))
        getattr(p["e4m3"], nm).view(torch.uint8)[0].copy_(q)
        getattr(p["e4m3"], nm + "s")[0].copy_(torch.ldexp(torch.ones(e.shape), e))
        getattr(p["bf16"], nm)[0].copy_(img)
        getattr(p["fp32"], nm)[0].copy_(img)
    seqs = [KVSeq(p["fp32"]) for _ in range(n_seq)]
    for s in seqs:   # L - tokens keys, the step appends the rest (values random)
        s.reserve(L - tokens)
        s.length = L - tokens
    meta = BatchMeta([(s, tokens, s.length, True) for s in seqs], dev, gqa=H // KVH, rows=ops.attn_item_rows(hd))
    T = meta.T
    q = torch.randn(T, H * hd, device=dev, generator=g)
    if graph:   # a captured step: capacity of at least 2048 keys, 128-key splits
        ns, kps = ops.attn_nsplit(max(2048, L + 64), meta.n_items, KVH), 128
    else:       # an eager forward sizes both per launch (DecoderStack.forward)
        ns, kps = ops.attn_nsplit(meta.max_keys, meta.n_items, KVH), ops.attn_keys_per_split(meta.max_keys, meta.n_items,
                                                                                             KVH, hd, dev)
    ml = torch.empty(T * H * ns * 2, device=dev)
    po = torch.empty(T * H * ns * hd, device=dev)
    tk = torch.zeros(meta.n_items * KVH, dtype=torch.int32, device=dev)
    outs = {a: torch.empty(T, H * hd, device=dev) for a in ARMS}
    dense = meta.n_items == T == meta.S or meta.uniform

    def launch(a):
        ops.attention(q, T, None if dense else meta.items, meta.n_items, meta.max_rows, meta.tok_nvis, meta.block_table,
                      PS, p[a].k[0], p[a].v[0], H, KVH, hd, hd ** -0.5, ns, ml, po, outs[a], tickets=tk,
                      keys_per_split=kps, **scales_of(p[a]))

    t = arms({a: (lambda a=a: launch(a)) for a in ARMS})
    ops.launch_counts_reset()
    launch("e4m3")
    torch.cuda.synchronize()
    kinds = "+".join(k for k, v in ops.launch_counts().items() if v)
    same = torch.equal(outs["e4m3"], outs["bf16"]) and torch.equal(outs["e4m3"], outs["fp32"])
    best = row(f"attention {name}", t, f"  items {meta.n_items} x {meta.max_rows} rows, nsplit {ns}, kps {kps}, {kinds}, "
               f"outputs {'equal' if same else 'DIFFER'}")
    for s in seqs:
        s.free()
    return best


def layout_tables():
    att = {}
    for L in (150, 448, 1000, 4000):
        att[L] = attention(f"text step 8 x 1 token, {L} keys", 8, 1, L, True)
    attention("listen chunk 8 x 2 tokens, 200 keys", 8, 2, 200, True)
    attention("duplex tick 8 x 4 tokens, 600 keys", 8, 4, 600, False)
    attention("8-chunk group 64 x 2 tokens, 200 keys", 64, 2, 200, True)

    # -------------------------------------------------------------- q|k|v projection + RoPE + append
    def pack_x(x, xp):
        M, K = x.shape
        full = torch.zeros(16 * xp.rb, K, device=dev)
        full[:M] = x
        hi = full.to(torch.bfloat16)
        lo = (full - hi.float()).to(torch.bfloat16)
        for src, dst in ((hi, xp.hi), (lo, xp.lo)):
            dst.copy_(src.view(xp.rb, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).reshape(-1))

    N = (H + 2 * KVH) * hd
    lin = ops.PackedLinear((torch.randn(N, D, device=dev, generator=g) * 0.02).to(torch.bfloat16),
                           torch.randn(N, device=dev, generator=g) * 0.5, rope_hd=hd)
    cos, sin = (t.to(dev) for t in tables.rope_tables(1e6, hd, 4096, round_fp16=True))
    a = pools(64)
    app = {}
    for M in (8, 16, 32, 128):
        x = torch.randn(M, D, device=dev, generator=g)
        slot = torch.randperm(64 * PS, device=dev, generator=g)[:M].to(torch.int32)
        pos = torch.randint(0, 4096, (M,), device=dev, generator=g, dtype=torch.int32)
        qo = torch.empty(M, H * hd, device=dev)
        k8 = torch.zeros(1, KVH, M, hd, device=dev)
        v8 = torch.zeros(1, KVH, M, hd, device=dev)
        slot8 = torch.arange(M, dtype=torch.int32, device=dev)
        xp = None
        if 8 < M <= 64:
            xp = ops.XPack(D, dev, M)
            pack_x(x, xp)

        def quantise():
            ops.kv8_append(k8, v8, M, slot, a["e4m3"].k[0], a["e4m3"].ks[0], a["e4m3"].v[0], a["e4m3"].vs[0], PS)

        def append(arm):
            if arm == "e4m3":   # DecoderStack.forward's FP8 path: the staging cache, then the append launch
                lin.qkv_rope(x, M, pos, slot8, cos, sin, qo, k8, v8, H, KVH, M, xpack=xp)
                quantise()
            else:
                lin.qkv_rope(x, M, pos, slot, cos, sin, qo, a[arm].k[0], a[arm].v[0], H, KVH, PS, xpack=xp)

        fns = {arm: (lambda arm=arm: append(arm)) for arm in ARMS}
        fns["kv8_append alone"] = quantise
        t = arms(fns)
        app[M] = row(f"q|k|v + append, {M} rows", t)
    # where the attention's gain over bf16 outgrows the append launch's cost at the text step (8 rows)
    cost = app[8]["e4m3"] - app[8]["bf16"]
    print(f"text step (8 rows): the staged append costs {cost:+.2f} us a layer over the bf16 pool's projection "
          f"(the launch alone {app[8]['kv8_append alone']:.2f} us); the attention gains over bf16: "
          + ", ".join(f"{L} keys {att[L]['bf16'] - att[L]['e4m3']:+.2f} us" for L in att), flush=True)


# ------------------------------------------------------------------ the B = 8 text step
def text_step():
    """One engine per pool (built one after the other: the arms are not alternated here), all weights under MXFP4; the
    same sessions are timed at ~150 keys and, their context extended, at ~4,000."""
    import gc
    from fo.engine import FreezeOmniEngine
    B, N = 8, 40
    for kv in ARMS:
        eng = FreezeOmniEngine(os.path.join(ROOT, "configs", "real"), device=dev, max_sessions=B, llm_kv=kv,
                               llm_kv_tokens=B * 4400, mlp_weights="mxfp4", lm_head_weights="mxfp4",
                               attn_weights="mxfp4")
        base = eng.system_role("<|im_start|>system\nYou are a helpful assistant.")
        kvs = [base.fork() for _ in range(B)]
        for keys in (150, 4000):
            while kvs[0].length < keys - 60:   # the context, in chunks of at most 128 tokens a session
                n = min(128, keys - 60 - kvs[0].length)
                eng.text_step([(s, list(range(100, 100 + n))) for s in kvs])
            ids, _ = eng.text_step([(s, [1]) for s in kvs])
            for _ in range(5):
                ids, _ = eng.text_step([(s, [i]) for s, i in zip(kvs, ids)])
            best = []
            for _ in range(REPEATS):
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(N):
                    ids, _ = eng.text_step([(s, [i]) for s, i in zip(kvs, ids)])
                torch.cuda.synchronize()
                best.append((time.perf_counter() - t) / N * 1e3)
            print(f"text step B={B} all-MXFP4 weights, llm_kv={kv}, {kvs[0].length} keys: {min(best):.3f} ms wall/step "
                  f"({' '.join(f'{x:.3f}' for x in best)}), {eng.llm.pool.bytes_per_token} B of cache a token",
                  flush=True)
        del eng, base, kvs
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "text":
        text_step()
    else:
        layout_tables()
