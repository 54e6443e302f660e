"""A/B of the 17..64-row MXFP4 weight stream (fo_gemm_w4_rows, PackedLinearW4(stream_rows=64)) against the bf16 arm on
the same model (k_gemm_xsk + reduce on the exact bf16 image of the MXFP4 weights, ops.PackedLinearW4.bf16 -- the kernels
an mxfp4 engine runs at these rows without the option) on the Qwen2 MLP shapes at M = 32, 48 and 64: gate/up (N 18,944,
K 3,584; SwiGLU + RMSNorm consumer) and down (N 3,584, K 18,944; + residual + next-norm statistics).  A third arm, for
information, is the FP8 row stream (fo_gemm_w8_rows) on the same source weights.  --fmt mxfp6 puts the MXFP6 row stream
(fo_gemm_w6_rows, PackedLinearW6(stream_rows=64)) in the MXFP4 arm's place, against the bf16 image of the MXFP6 weights,
with the FP8 and MXFP4 row streams on the same source weights for information.  The method is
scripts/gemm_w8_rows_ab.py's: per-launch device time from one replayed hipGraph of launches that walk weight copies
larger than the 256 MB Infinity Cache in every arm, the arms alternated in one process, three repeats each so the spread
shows, and an output check of MXFP4 against bf16.  The launches of one call of each arm are printed first, so the record
shows which kernels were timed.  Last, the q|k|v projection (+ RoPE + KV append, RMSNorm consumer) at 32 rows reading
its input packed (ops.XPack, filled by a bf16 down) against reading the fp32 rows: what the stack gives up when an
MXFP4 down, which writes no packed x * gamma, feeds it.
The rule: a (GEMM, row blocks) pair belongs in ops.W4_ROWS_POLICY only if the MXFP4 arm's median beats the
bf16 arm's median by more than the bf16 arm's repeat-to-repeat spread (max - min) at that pair -- for the down, by more
than that spread plus the packed-input cost of the q|k|v; the summary at the end applies it.
python scripts/gemm_w4_rows_ab.py [--fmt mxfp4|mxfp6] [rows ...] (GPU only; default mxfp4, rows 32 48 64)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_graph_sweep_util import graph_time  # noqa: E402
from fo import ops  # noqa: E402
from fo.ops import QUANT_LINEAR, PackedLinear  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--fmt", choices=("mxfp4", "mxfp6"), default="mxfp4", help="the format under test")
ap.add_argument("rows", nargs="*", type=int)
args = ap.parse_args()
FMT = args.fmt
INFO = ("fp8",) if FMT == "mxfp4" else ("fp8", "mxfp4")   # the row streams timed for information
ROWS = args.rows or [32, 48, 64]
dev = torch.device("cuda:0")
D, I = 3584, 18944
g = torch.Generator(device=dev).manual_seed(0)
PEAK = 8.0e12
ARMS = ("bf16", FMT) + INFO
POLICY_NAME = {"mxfp4": "W4_ROWS_POLICY", "mxfp6": "W6_ROWS_POLICY"}[FMT]


def rnd(*s, scale=0.02):
    return torch.randn(*s, device=dev, generator=g) * scale


class Arms:
    """One weight under the arms: the layer of the format under test (row stream forced), its bf16 image, and the
    layers of the formats timed for information (row stream forced) on the same source weight."""

    def __init__(self, w, up=None):
        self.nbytes = {}
        for fmt in (FMT,) + INFO:
            lin = QUANT_LINEAR[fmt](w, swiglu_up=up, stream_rows=64)
            lin.rows_rb = (2, 3, 4)   # every 17..64-row call on the row stream, whatever the policy says
            setattr(self, fmt, lin)
            self.nbytes[fmt] = lin.code_nbytes(fmt)
        self.bf16 = getattr(self, FMT).bf16
        self.nbytes["bf16"] = self.bf16.nbytes


def kinds(fn):
    ops.launch_counts_reset()
    ops.w4_launch_counts_reset()
    ops.w6_launch_counts_reset()
    fn()
    c = {k: v for k, v in ops.launch_counts().items() if v}
    if ops.w4_rows_launch_count():
        c["fo_gemm_w4_rows calls"] = ops.w4_rows_launch_count()
    if ops.w6_rows_launch_count():
        c["fo_gemm_w6_rows calls"] = ops.w6_rows_launch_count()
    return c


SUMMARY = []


def ab(name, make, ncp, M, nbytes):
    res = {a: [] for a in ARMS}
    outs = {}
    for arm in ARMS:
        print(f"{name:14s} M={M:2d}  {arm} launches of one call: {kinds(make(0, arm))}", flush=True)
    for _ in range(3):
        for arm in ARMS:
            fns = [make(i, arm) for i in range(ncp)]
            it = iter(range(1 << 30))
            res[arm].append(graph_time(lambda: fns[next(it) % ncp](), ncp * max(1, 48 // ncp)))
            o = fns[0](check=True)
            torch.cuda.synchronize()
            outs[arm] = [t.clone() for t in o]
    err = max(float((x - y).abs().max() / (x.abs().max() + 1e-30)) for x, y in zip(outs["bf16"], outs[FMT]))
    med = {a: statistics.median(res[a]) for a in ARMS}
    spread = max(res["bf16"]) - min(res["bf16"])
    fmt = lambda v: "/".join(f"{t:.1f}" for t in v)   # noqa: E731
    print(f"{name:14s} M={M:2d}  " +
          "  ".join(f"{a} {fmt(res[a])} us (median {med[a]:.1f}, {nbytes[a] / 1e6:.0f} MB, "
                    f"{nbytes[a] / med[a] / 1e6:4.2f} TB/s)" for a in ARMS) +
          f"  {FMT}/bf16 {med[FMT] / med['bf16']:.3f}  " +
          "  ".join(f"{FMT}/{a} {med[FMT] / med[a]:.3f}" for a in INFO) +
          f"  bf16 spread {spread:.1f} us  rel diff {FMT} vs bf16 {err:.2e}", flush=True)
    SUMMARY.append((name, M, med["bf16"], med[FMT], {a: med[a] for a in INFO}, spread))


# copies: bf16 images 4 x 272 MB / 6 x 136 MB, FP8 codes half, MXFP6 codes + scales 0.39, MXFP4 a quarter + 1/32
NG, ND = 4, 6
gus = [Arms(rnd(I, D).to(torch.bfloat16), rnd(I, D).to(torch.bfloat16)) for _ in range(NG)]
downs = [Arms(rnd(D, I).to(torch.bfloat16)) for _ in range(ND)]
stats = ops.RowStats(64, dev)
for M in ROWS:
    xg, res0, yg = rnd(M, D, scale=1.0), rnd(M, D, scale=1.0), torch.empty(M, D, device=dev)
    # producer statistics for the gate/up consumer (a down projection with stats_out)
    downs[0].bf16(rnd(M, I, scale=1.0), out=res0.clone(), residual=True, M=M,
                  stats_out=stats.set(torch.ones(D, device=dev), yg))
    outs = [torch.empty(M, I, device=dev) for _ in range(NG)]

    def mk_gu(i, arm, M=M, outs=outs, yg=yg):
        lin = getattr(gus[i], arm)

        def f(check=False):
            return [lin(yg, out=outs[i], M=M, norm=(stats, 1e-6))]
        return f
    ab("gate/up+rms", mk_gu, NG, M, gus[0].nbytes)

    xm = rnd(M, I, scale=1.0)
    ys = [res0.clone() for _ in range(ND)]
    ygs = [torch.empty(M, D, device=dev) for _ in range(ND)]
    st = [ops.RowStats(64, dev) for _ in range(ND)]
    gam = torch.rand(D, device=dev, generator=g) + 0.5

    def mk_down(i, arm, M=M, xm=xm, ys=ys, ygs=ygs, st=st, gam=gam, res0=res0):
        lin = getattr(downs[i], arm)

        def f(check=False):
            if check:
                ys[i].copy_(res0)
            lin(xm, out=ys[i], residual=True, M=M, stats_out=st[i].set(gam, ygs[i]))
            return [ys[i], ygs[i]]
        return f
    ab("down+res+stats", mk_down, ND, M, downs[0].nbytes)

# q|k|v at 32 rows: packed X (written by the producing bf16 down) against the fp32 rows
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
cost = max(0.0, statistics.median(res["fp32 rows"]) - statistics.median(res["packed"]))
print(f"packed-input cost handed to the next q|k|v: {cost:.1f} us (medians)", flush=True)

print(f"\nthe rule: (GEMM, row blocks) -> bf16 median - {FMT} median against the margin to beat (us)")
policy = {"gate_up": [], "down": []}
for name, M, b, m, info, spread in SUMMARY:
    key = "down" if name.startswith("down") else "gate_up"
    margin = spread + (cost if key == "down" else 0.0)
    wins = b - m > margin
    if wins:
        policy[key].append((M + 15) // 16)
    print(f"{name:14s} M={M:2d}  gain {b - m:+6.1f}  margin {margin:5.1f}  {'ENTERS' if wins else 'stays on the image'}"
          f"   (for information: " + ", ".join(f"{a} row stream {b - t:+6.1f}" for a, t in info.items()) + ")")
print(f"{POLICY_NAME} =", {k: tuple(v) for k, v in policy.items()}, flush=True)
