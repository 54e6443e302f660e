"""The Qwen2 text step's attention (fo_attention: 28 q / 4 kv heads of 128, 8 sessions x 1 token, the TextGraph's
16 split slots of 128 keys with the in-launch merge) against the context length L: device time per launch (replayed
hipGraph, 50 launches) and the error against a torch fp32 reference.  Run once per library (FO_LIB_PATH picks an
older build) to place GQA_DEC_KEYS (fo_attn.hip): the single-row body serves an item up to that many keys, the
multi-row split body beyond.
python scripts/attn_gqa_crossover.py [L,L,...] (GPU only)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_graph_sweep_util import graph_time  # noqa: E402
from fo import _lib, ops  # noqa: E402
from fo.kv import BatchMeta, KVPool, KVSeq  # noqa: E402

dev = torch.device("cuda:0")
H, KVH, hd, B = 28, 4, 128, 8
LS = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else \
    [64, 128, 150, 192, 230, 256, 320, 384, 448, 512, 513, 640, 768, 1024]
pool = KVPool(1, KVH, hd, 1024, 16, dev)
g = torch.Generator(device=dev).manual_seed(0)
print(f"library {_lib.LIB_PATH}", flush=True)
for L in LS:
    seqs = [KVSeq(pool) for _ in range(B)]
    for s in seqs:   # L - 1 keys, the step appends one (values random)
        s.reserve(L - 1)
        s.length = L - 1
    pool.k[0].normal_(generator=g)
    pool.v[0].normal_(generator=g)
    meta = BatchMeta([(s, 1, s.length, True) for s in seqs], dev, gqa=H // KVH)
    q = torch.randn(B, H * hd, device=dev, generator=g)
    out = torch.empty(B, H * hd, device=dev)
    ref = torch.empty(B, H * hd, device=dev)
    for b, sq in enumerate(seqs):
        Kb = pool.k[0][sq.pages].permute(1, 0, 2, 3).reshape(KVH, -1, hd)[:, :L]
        Vb = pool.v[0][sq.pages].permute(1, 0, 2, 3).reshape(KVH, -1, hd)[:, :L]
        sc = torch.einsum("gjd,gkd->gjk", q[b].view(KVH, H // KVH, hd), Kb) * hd ** -0.5
        ref[b] = torch.einsum("gjk,gkd->gjd", sc.softmax(-1), Vb).reshape(-1)
    ns = ops.attn_nsplit(2048, B, KVH)
    ml = torch.empty(B * H * ns * 2, device=dev)
    po = torch.empty(B * H * ns * hd, device=dev)
    tk = torch.zeros(B * KVH, dtype=torch.int32, device=dev)

    def f():
        ops.attention(q, B, None, B, meta.max_rows, meta.tok_nvis, meta.block_table, pool.PS, pool.k[0], pool.v[0], H,
                      KVH, hd, hd ** -0.5, ns, ml, po, out, tickets=tk, keys_per_split=128)
    ts = [graph_time(f, 50) for _ in range(3)]
    ops.launch_counts_reset()
    f()
    torch.cuda.synchronize()
    kinds = [k for k, v in ops.launch_counts().items() if v]
    print(f"L={L:5d} nsplit={ns}: {min(ts):6.2f} us (3 repeats: {' '.join(f'{t:.2f}' for t in ts)})  err "
          f"{(out - ref).abs().max().item():.1e}  {'+'.join(kinds)}", flush=True)
    for s in seqs:
        s.free()
