"""A/B of the 17..64-row FP8 weight stream (fo_gemm_w8_rows, PackedLinearW8(stream_rows=64)) or, with --band 128, of
the 65..128-row one (fo_gemm_w8_rows128, stream_rows=128) against the bf16 arm on the same model (k_gemm_xsk + reduce,
at 65..128 rows k_gemm_rows + k_gemm_reduce, on the exact bf16 image of the FP8 weights, ops.PackedLinearW8.bf16 -- the
kernels a bf16 engine runs) on the Qwen2 MLP shapes at M = 32, 48 and 64 (80, 96, 112 and 128): gate/up (N 18,944,
K 3,584; SwiGLU + RMSNorm consumer) and down (N 3,584, K 18,944; + residual + next-norm statistics).  The method is
scripts/gemm_w8_ab.py's: per-launch device time from one replayed hipGraph of launches that walk weight copies larger
than the 256 MB Infinity Cache in both arms, the arms alternated in one process, three repeats each so the spread shows,
and an output check of FP8 against bf16.  The launch kinds of one call of each arm are printed first, so the record
shows which kernels were timed.  A (GEMM, row blocks) pair belongs in ops.W8_ROWS_POLICY only if fp8 beats bf16 in every
repeat by more than the bf16 arm's spread: the last column says so.  Last, for band 64, the q|k|v projection (+ RoPE +
KV append, RMSNorm consumer) at 32 rows reading its input packed (ops.XPack, filled by a bf16 down) against reading the
fp32 rows: what the stack gives up when an FP8 down, which writes no packed x * gamma, feeds it.
python scripts/gemm_w8_rows_ab.py [--band 64|128] [rows ...] (GPU only; default band 64, rows 32 48 64 / 80 96 112 128)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_graph_sweep_util import graph_time  # noqa: E402
from fo import ops  # noqa: E402
from fo.ops import PackedLinearW8  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--band", type=int, choices=(64, 128), default=64)
ap.add_argument("rows", type=int, nargs="*")
args = ap.parse_args()
BAND, MW = args.band, len(str(args.band))   # (MW: the width M is printed at, as the records of each band have it)
dev = torch.device("cuda:0")
D, I = 3584, 18944
g = torch.Generator(device=dev).manual_seed(0)
PEAK = 8.0e12


def rnd(*s, scale=0.02):
    return torch.randn(*s, device=dev, generator=g) * scale


def w8(w, up=None):
    lin = PackedLinearW8(w, swiglu_up=up, stream_rows=BAND)
    lin.rows_rb = tuple(range(2, 9))   # every call of 17 rows up to the band on the FP8 streams, whatever the policy says
    return lin


def kinds(fn):
    ops.launch_counts_reset()
    fn()
    return {k: v for k, v in ops.launch_counts().items() if v}


def ab(name, make, ncp, M, bytes16, bytes8):
    res = {"bf16": [], "fp8": []}
    outs = {}
    for arm in ("bf16", "fp8"):
        print(f"{name:14s} M={M:{MW}d}  {arm} launches of one call: {kinds(make(0, arm))}", flush=True)
    for _ in range(3):
        for arm in ("bf16", "fp8"):
            fns = [make(i, arm) for i in range(ncp)]
            it = iter(range(1 << 30))
            res[arm].append(graph_time(lambda: fns[next(it) % ncp](), ncp * max(1, 48 // ncp)))
            o = fns[0](check=True)
            torch.cuda.synchronize()
            outs[arm] = [t.clone() for t in o]
    err = max(float((x - y).abs().max() / (x.abs().max() + 1e-30)) for x, y in zip(outs["bf16"], outs["fp8"]))
    t16, t8 = min(res["bf16"]), min(res["fp8"])
    spread = (max(res["bf16"]) - t16) / t16
    fmt = lambda v: "/".join(f"{t:.1f}" for t in v)   # noqa: E731
    print(f"{name:14s} M={M:{MW}d}  bf16 {fmt(res['bf16'])} us ({bytes16 / 1e6:.0f} MB, {bytes16 / t16 / 1e6:4.2f} TB/s)  "
          f"fp8 {fmt(res['fp8'])} us ({bytes8 / 1e6:.0f} MB, {bytes8 / t8 / 1e6:4.2f} TB/s, "
          f"{bytes8 / PEAK * 1e6 / t8:4.2f} of the {bytes8 / PEAK * 1e6:.1f} us floor)  fp8/bf16 {t8 / t16:.3f}  "
          f"bf16 spread {spread:.3f}  rel diff {err:.2e}  "
          f"{'WINS' if max(res['fp8']) < t16 * (1 - spread) else 'stays on the image'}", flush=True)


NG, ND = 4, 6   # copies: FP8 codes 4 x 136 MB / 6 x 68 MB, bf16 images twice that
gus = [w8(rnd(I, D).to(torch.bfloat16), rnd(I, D).to(torch.bfloat16)) for _ in range(NG)]
downs = [w8(rnd(D, I).to(torch.bfloat16)) for _ in range(ND)]
stats = ops.RowStats(BAND, dev)
for M in (args.rows or {64: [32, 48, 64], 128: [80, 96, 112, 128]}[BAND]):
    xg, res0, yg = rnd(M, D, scale=1.0), rnd(M, D, scale=1.0), torch.empty(M, D, device=dev)
    # producer statistics for the gate/up consumer (a down projection with stats_out)
    downs[0].bf16(rnd(M, I, scale=1.0), out=res0.clone(), residual=True, M=M,
                  stats_out=stats.set(torch.ones(D, device=dev), yg))
    outs = [torch.empty(M, I, device=dev) for _ in range(NG)]

    def mk_gu(i, arm, M=M, outs=outs, yg=yg):
        lin = gus[i] if arm == "fp8" else gus[i].bf16

        def f(check=False):
            return [lin(yg, out=outs[i], M=M, norm=(stats, 1e-6))]
        return f
    ab("gate/up+rms", mk_gu, NG, M, gus[0].nbytes, gus[0].fp8_nbytes)

    xm = rnd(M, I, scale=1.0)
    ys = [res0.clone() for _ in range(ND)]
    ygs = [torch.empty(M, D, device=dev) for _ in range(ND)]
    st = [ops.RowStats(BAND, dev) for _ in range(ND)]
    gam = torch.rand(D, device=dev, generator=g) + 0.5

    def mk_down(i, arm, M=M, xm=xm, ys=ys, ygs=ygs, st=st, gam=gam, res0=res0):
        lin = downs[i] if arm == "fp8" else downs[i].bf16

        def f(check=False):
            if check:
                ys[i].copy_(res0)
            lin(xm, out=ys[i], residual=True, M=M, stats_out=st[i].set(gam, ygs[i]))
            return [ys[i], ygs[i]]
        return f
    ab("down+res+stats", mk_down, ND, M, downs[0].nbytes, downs[0].fp8_nbytes)

if BAND != 64:
    sys.exit(0)
# q|k|v at 32 rows: packed X (written by the producing bf16 down) against the fp32 rows
from fo.ops import PackedLinear  # noqa: E402
H, KVH, hd, M = 28, 4, 128, 32
qkvs = [PackedLinear(rnd(H * hd + 2 * KVH * hd, D).to(torch.bfloat16), rnd(H * hd + 2 * KVH * hd), rope_hd=hd)
        for _ in range(6)]
cos = torch.rand(4096, hd // 2, device=dev, generator=g)
sin = torch.rand(4096, hd // 2, device=dev, generator=g)
PS, pages = 16, 64
kc = torch.zeros(pages, KVH, PS, hd, device=dev)
vc = torch.zeros_like(kc)
pos = torch.arange(100, 100 + M, dtype=torch.int32, device=dev)
slot = torch.arange(5, 5 + M, dtype=torch.int32, device=dev)
qo = torch.empty(M, H * hd, device=dev)
xp = ops.XPack(D, dev, M)
xq = torch.empty(M, D, device=dev)
downs[0].bf16(rnd(M, I, scale=1.0), out=rnd(M, D, scale=1.0), residual=True, M=M,
              stats_out=stats.set(torch.ones(D, device=dev), xq), ypack=xp)
res = {"packed": [], "fp32 rows": []}
for _ in range(3):
    for arm, pk in (("packed", xp), ("fp32 rows", None)):
        it = iter(range(1 << 30))
        res[arm].append(graph_time(lambda: qkvs[next(it) % 6].qkv_rope(xq, M, pos, slot, cos, sin, qo, kc, vc, H, KVH, PS,
                                                                       norm=(stats, 1e-6), xpack=pk), 48))
print("q|k|v+rope     M=32  " + "  ".join(f"{k} {'/'.join(f'{t:.1f}' for t in v)} us" for k, v in res.items()), flush=True)
