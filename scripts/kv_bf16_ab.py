"""The bf16 paged-KV layout (llm_kv="bf16") against the fp32 one on the Qwen2 shapes (28 q / 4 kv heads of
128, pages of 16): both pools in one process holding the same (bf16-representable) values, the two arms alternated,
every figure the per-launch device time of 50 launches captured as one hipGraph and replayed, three repeats per arm.

fo_attention at
  the text step       8 x 1 token  at 150, 448, 1,000 and 4,000 keys (the TextGraph's launch: tickets, 128-key splits)
  the same step       at 384, 448 and 512 keys forced onto the multi-row body (where GQA_DEC_KEYS belongs per layout)
  the listen chunk    8 x 2 tokens at 200 keys (the ListenGraph's launch)
  the duplex tick     8 x 4 tokens at 600 keys (the eager launch: 16 items of 2 tokens, keys per split sized per launch)
  the 8-chunk group   64 items x 2 tokens at 200 keys (64 sequences here; the group's items are 8 sessions x 8 chunks)
and the q|k|v projection + RoPE + append (K = 3584, synthetic weights) at 8, 16, 32 and 128 rows (16 and 32 rows on
packed X, as layers > 0 of a forward read it).

A replayed launch re-reads the same K / V, so what it reads sits in the L2 / Infinity Cache as far as it fits there
(the text step at 4,000 keys: 8 sessions x 4 kv heads x 4,000 keys x 128 x (K + V) = 131 MB fp32 / 66 MB bf16 per
launch).  Each attention row also reports whether the two arms' outputs are equal (they must be).

python scripts/kv_bf16_ab.py (GPU only)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_graph_sweep_util import graph_time  # noqa: E402
from fo import _lib, ops, tables  # noqa: E402
from fo.kv import BatchMeta, KVPool, KVSeq  # noqa: E402

dev = torch.device("cuda:0")
H, KVH, hd, PS, D = 28, 4, 128, 16, 3584
REPS, REPEATS = 50, 3
g = torch.Generator(device=dev).manual_seed(0)
print(f"library {_lib.LIB_PATH}", flush=True)


def arms(f32, f16):
    """Three repeats of each arm, alternated; -> (fp32 times, bf16 times) in us."""
    t32, t16 = [], []
    for _ in range(REPEATS):
        t32.append(graph_time(f32, REPS))
        t16.append(graph_time(f16, REPS))
    return t32, t16


def row(name, t32, t16, extra=""):
    a, b = min(t32), min(t16)
    print(f"{name:44s} fp32 {a:7.2f} us ({' '.join(f'{t:.2f}' for t in t32)}; spread {max(t32) - a:.2f})   "
          f"bf16 {b:7.2f} us ({' '.join(f'{t:.2f}' for t in t16)}; spread {max(t16) - b:.2f})   "
          f"bf16 / fp32 {b / a:.3f} {extra}", flush=True)


# ------------------------------------------------------------------ fo_attention
def attention(name, n_seq, tokens, L, graph, rows=None):
    """rows: the launch's max_rows when not the items' own (one token per session with max_rows 8 instead of 7 takes
    k_attn_mfma<128, 8>, the multi-row body, at any key count: the other side of GQA_DEC_KEYS)."""
    n_pages = n_seq * ((L + PS - 1) // PS) + 1
    p32 = KVPool(1, KVH, hd, n_pages, PS, dev)
    p16 = KVPool(1, KVH, hd, n_pages, PS, dev, dtype=torch.bfloat16)
    for nm in ("k", "v"):
        getattr(p16, nm).normal_(generator=g)
        getattr(p32, nm).copy_(getattr(p16, nm))
    seqs = [KVSeq(p32) for _ in range(n_seq)]
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
    outs = {4: torch.empty(T, H * hd, device=dev), 2: torch.empty(T, H * hd, device=dev)}
    dense = meta.n_items == T == meta.S or meta.uniform

    def launch(pool, out):
        ops.attention(q, T, None if dense else meta.items, meta.n_items, rows or meta.max_rows, meta.tok_nvis,
                      meta.block_table,
                      PS, pool.k[0], pool.v[0], H, KVH, hd, hd ** -0.5, ns, ml, po, out, tickets=tk, keys_per_split=kps)

    t32, t16 = arms(lambda: launch(p32, outs[4]), lambda: launch(p16, outs[2]))
    ops.launch_counts_reset()
    launch(p16, outs[2])
    torch.cuda.synchronize()
    kinds = "+".join(k for k, v in ops.launch_counts().items() if v)
    row(f"attention {name}", t32, t16, f"  items {meta.n_items} x {meta.max_rows} rows, nsplit {ns}, kps {kps}, {kinds}, "
        f"outputs {'equal' if torch.equal(outs[4], outs[2]) else 'DIFFER'}")
    for s in seqs:
        s.free()


for L in (150, 448, 1000, 4000):
    attention(f"text step 8 x 1 token, {L} keys", 8, 1, L, True)
# the single-row body against the multi-row one around GQA_DEC_KEYS = 448 (the single-row body serves <= 512 keys)
for L in (384, 448, 512):
    attention(f"text step, {L} keys, multi-row body", 8, 1, L, True, rows=8)
attention("text step, 512 keys (multi-row by count)", 8, 1, 512, True)
attention("listen chunk 8 x 2 tokens, 200 keys", 8, 2, 200, True)
attention("duplex tick 8 x 4 tokens, 600 keys", 8, 4, 600, False)
attention("8-chunk group 64 x 2 tokens, 200 keys", 64, 2, 200, True)


# ------------------------------------------------------------------ q|k|v projection + RoPE + append
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
a32 = KVPool(1, KVH, hd, 64, PS, dev)
a16 = KVPool(1, KVH, hd, 64, PS, dev, dtype=torch.bfloat16)
for M in (8, 16, 32, 128):
    x = torch.randn(M, D, device=dev, generator=g)
    slot = torch.randperm(64 * PS, device=dev, generator=g)[:M].to(torch.int32)
    pos = torch.randint(0, 4096, (M,), device=dev, generator=g, dtype=torch.int32)
    qo = torch.empty(M, H * hd, device=dev)
    xp = None
    if 8 < M <= 64:
        xp = ops.XPack(D, dev, M)
        pack_x(x, xp)

    def append(pool):
        lin.qkv_rope(x, M, pos, slot, cos, sin, qo, pool.k[0], pool.v[0], H, KVH, PS, xpack=xp)

    t32, t16 = arms(lambda: append(a32), lambda: append(a16))
    ops.launch_counts_reset()
    append(a16)
    torch.cuda.synchronize()
    kinds = "+".join(k for k, v in ops.launch_counts().items() if v)
    row(f"q|k|v + append, {M} rows", t32, t16, f"  {kinds}")
