"""A/B of the quantised Qwen2 attention projections at <= 16 rows: the fused q|k|v (4608 x 3584, with the RMSNorm consumer,
bias, RoPE and the paged-KV append) and o (3584 x 3584, with the residual and the RMSNorm producer) at M = 1, 8 and 16,
three arms each: the exact bf16 image of the FP8 W' on today's kernel as the engine calls it (at 9..16 rows it reads the
packed input its producer wrote, and o writes the packed x * gamma), the FP8 stream (fo_gemm_w8_qkv_rope / fo_gemm_w8) and
the MXFP4 stream (fo_gemm_w4_qkv_rope / fo_gemm_w4), which read fp32 rows and write none packed.  The method is
scripts/gemm_head_ab.py's: per-launch device time from one replayed hipGraph, the arms alternated in one process, three
repeats each so the spread shows, and an output check of each stream against its own image.  These weights are 7-33 MB,
so every arm cycles over enough distinct copies that one cycle exceeds twice the 256 MB Infinity Cache in that arm's own
format: no launch finds its weight in cache, as no layer of a real step does.  ops.ATTN_POLICY's rule (DESIGN 5.5's): a
(format, GEMM) pair streams its codes only if, at both 8 and 16 rows, its median beats the bf16 arm's median by more
than that arm's repeat-to-repeat spread (max - min); the last lines say so.
python scripts/gemm_attn_ab.py [rows ...] (GPU only)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_graph_sweep_util import graph_time  # noqa: E402
from fo import ops, tables  # noqa: E402
from fo.kv import KVPool  # noqa: E402
from fo.ops import PackedLinear, PackedLinearW4, PackedLinearW8, PackedQKVQuant  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("rows", type=int, nargs="*")
args = ap.parse_args()
dev = torch.device("cuda:0")
D, H, KVH, HD, PS, EPS = 3584, 28, 4, 128, 16, 1e-6
NQ = (H + 2 * KVH) * HD
CYCLE = 2 * 256e6
g = torch.Generator(device=dev).manual_seed(0)
ARMS = ("bf16", "fp8", "mxfp4")
verdict = {(a, k): {} for a in ARMS[1:] for k in ("qkv", "o")}


def rnd(*s, scale=0.02):
    return torch.randn(*s, device=dev, generator=g) * scale


def qkv(fmt):
    lin = PackedQKVQuant(rnd(NQ, D).to(torch.bfloat16), rnd(NQ, scale=0.5), HD, fmt)
    lin.stream = True   # on the stream whatever the policy says
    return lin


def o(cls):
    lin = cls(rnd(D, D).to(torch.bfloat16), kind="attn_o")
    lin.stream = True
    return lin


def copies(make, own):
    """Enough distinct copies that one cycle exceeds CYCLE bytes of `own(lin)`."""
    out = [make()]
    while own(out[0]) * len(out) <= CYCLE:
        out.append(make())
    torch.cuda.empty_cache()
    return out


def kinds(fn):
    ops.launch_counts_reset()
    ops.w4_launch_counts_reset()
    ops.qkv_quant_launch_counts_reset()
    fn()
    c = dict(ops.launch_counts(), **ops.w4_launch_counts(), **ops.qkv_quant_launch_counts())
    return {k: v for k, v in c.items() if v}


own = {"fp8": lambda lin: lin.fp8_nbytes, "mxfp4": lambda lin: lin.fp4_nbytes, "bf16": lambda lin: lin.nbytes}
lins = {"qkv": {"fp8": copies(lambda: qkv("fp8"), own["fp8"]), "mxfp4": copies(lambda: qkv("mxfp4"), own["mxfp4"])},
        "o": {"fp8": copies(lambda: o(PackedLinearW8), own["fp8"]), "mxfp4": copies(lambda: o(PackedLinearW4), own["mxfp4"])}}
for k in lins:   # the bf16 arm: the images of the FP8 copies, and as many more as its own cycle needs
    imgs = [lin.bf16 for lin in lins[k]["fp8"]]
    n = int(CYCLE // imgs[0].nbytes) + 1
    while len(imgs) < n:
        imgs.append((qkv("fp8") if k == "qkv" else o(PackedLinearW8)).bf16)
    lins[k]["bf16"] = imgs[:n]
    torch.cuda.empty_cache()
    b = {a: own[a](lins[k][a][0]) for a in ARMS}
    print(f"{k}: bf16 image {b['bf16'] / 1e6:.1f} MB x {len(lins[k]['bf16'])} copies, FP8 codes + scales "
          f"{b['fp8'] / 1e6:.1f} MB x {len(lins[k]['fp8'])}, MXFP4 codes + scales {b['mxfp4'] / 1e6:.1f} MB x "
          f"{len(lins[k]['mxfp4'])}", flush=True)
cos, sin = (t.to(dev) for t in tables.rope_tables(1e6, HD, 4096, round_fp16=True))
pool = KVPool(1, KVH, HD, 64, PS, dev)
for M in args.rows or [1, 8, 16]:
    # the q|k|v input as the engine has it: the previous down's x * gamma with its row statistics (and, at 9..16 rows,
    # the packed copy the bf16 arm reads); the o input: the attention's output (packed too at 9..16 rows)
    packs = M > 8
    sA, sB = ops.RowStats(16, dev), ops.RowStats(16, dev)
    gamma = 1 + rnd(D, scale=0.1)
    xg, res, xgp = torch.empty(M, D, device=dev), torch.empty(M, D, device=dev), ops.XPack(D, dev, M) if packs else None
    PackedLinear(rnd(D, 64, scale=0.125).to(torch.bfloat16))(rnd(M, 64, scale=1.0), out=res, M=M,
                                                            stats_out=sA.set(gamma, xg), ypack=xgp)
    att, attp = torch.empty(M, D, device=dev), ops.XPack(D, dev, M) if packs else None
    PackedLinear(rnd(D, 64, scale=0.125).to(torch.bfloat16))(      # (gamma 1: att = the product, packed beside it)
        rnd(M, 64, scale=1.0), out=torch.empty(M, D, device=dev), M=M,
        stats_out=ops.RowStats(16, dev).set(torch.ones(D, device=dev), att), ypack=attp)
    torch.cuda.synchronize()
    pos = torch.randint(0, 4096, (M,), device=dev, dtype=torch.int32, generator=g)
    slot = torch.randperm(64 * PS, device=dev, generator=g)[:M].to(torch.int32)
    q_out, x_out, yg, ygp = (torch.empty(M, H * HD, device=dev), torch.empty(M, D, device=dev),
                             torch.empty(M, D, device=dev), ops.XPack(D, dev, M) if packs else None)

    def call(kind, arm, i):
        lin = lins[kind][arm][i]
        image = arm == "bf16"
        if kind == "qkv":
            return lambda: lin.qkv_rope(xg, M, pos, slot, cos, sin, q_out, pool.k[0], pool.v[0], H, KVH, PS,
                                        norm=(sA, EPS), xpack=xgp if image else None)
        return lambda: lin(att, out=x_out, residual=True, M=M, stats_out=sB.set(gamma, yg),
                           xpack=attp if image else None, ypack=ygp if image else None)

    for kind in ("qkv", "o"):
        res_t = {a: [] for a in ARMS}
        for arm in ARMS:
            print(f"{kind} M={M:2d}  {arm} launches of one call: {kinds(call(kind, arm, 0))}", flush=True)
        for _ in range(3):
            for arm in ARMS:
                n = len(lins[kind][arm])
                fns = [call(kind, arm, i) for i in range(n)]
                it = iter(range(1 << 30))
                res_t[arm].append(graph_time(lambda: fns[next(it) % n](), 2 * n))
        err = {}
        for arm in ARMS[1:]:   # each stream against its own image
            lin = lins[kind][arm][0]
            if kind == "qkv":
                a = lin.qkv_rope(xg, M, pos, slot, cos, sin, torch.empty_like(q_out), pool.k[0], pool.v[0], H, KVH, PS,
                                 norm=(sA, EPS))
                b = lin.bf16.qkv_rope(xg, M, pos, slot, cos, sin, torch.empty_like(q_out), pool.k[0], pool.v[0], H, KVH,
                                      PS, norm=(sA, EPS))
            else:
                a, b = lin(att, M=M), lin.bf16(att, M=M)
            torch.cuda.synchronize()
            err[arm] = float((a - b).abs().max() / b.abs().max())
        med = {a: statistics.median(res_t[a]) for a in ARMS}
        spread = max(res_t["bf16"]) - min(res_t["bf16"])
        fmt = lambda v: "/".join(f"{t:.1f}" for t in v)   # noqa: E731
        cell = lambda a: (f"{a} {fmt(res_t[a])} us "   # noqa: E731
                          f"({own[a](lins[kind][a][0]) / med[a] / 1e6:4.2f} TB/s)")
        line = f"{kind} M={M:2d}  {cell('bf16')}  {cell('fp8')}  {cell('mxfp4')}  bf16 spread {spread:.1f} us"
        for arm in ARMS[1:]:
            wins = med[arm] < med["bf16"] - spread
            verdict[(arm, kind)][M] = wins
            line += (f"  {arm}/bf16 {med[arm] / med['bf16']:.3f} ({'WINS' if wins else 'does not win'}, rel diff to its "
                     f"image {err[arm]:.2e})")
        print(line, flush=True)
for (arm, kind), v in verdict.items():
    if 8 in v and 16 in v:
        ok = v[8] and v[16]
        print(f"{arm} {kind}: ATTN_POLICY {ok} -- {'streams the codes at <= 16 rows' if ok else 'runs the bf16 image at every row count'} "
              f"(wins at 8 rows: {v[8]}, at 16 rows: {v[16]})", flush=True)
