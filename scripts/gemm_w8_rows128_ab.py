"""A/B of the 65..128-row FP8 weight stream (fo_gemm_w8_rows128: k_w8_rows128 + k_w8_rows_merge,
PackedLinearW8(stream_rows=128)) against the bf16 arm on the same model (k_gemm_rows + k_gemm_reduce on the exact bf16
image of the FP8 weights, ops.PackedLinearW8.bf16 -- the kernels a bf16 engine runs) on the Qwen2 MLP shapes at
M = 80, 96, 112 and 128: gate/up (N 18,944, K 3,584; SwiGLU + RMSNorm consumer) and down (N 3,584, K 18,944;
+ residual + next-norm statistics).  The method is scripts/gemm_w8_rows_ab.py's: per-launch device time from one
replayed hipGraph of launches that walk weight copies larger than the 256 MB Infinity Cache in both arms, the arms
alternated in one process, three repeats each so the spread shows, and an output check of FP8 against bf16.  A (GEMM,
row blocks) pair belongs in ops.W8_ROWS_POLICY only if fp8 beats bf16 in every repeat by more than the bf16 arm's
spread: the last column says so.  The launch kinds of one call of each arm are printed first, so the record shows which
kernels were timed.
python scripts/gemm_w8_rows128_ab.py [rows ...] (GPU only; default rows 80 96 112 128)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_graph_sweep_util import graph_time  # noqa: E402
from fo import ops  # noqa: E402
from fo.ops import PackedLinearW8  # noqa: E402

dev = torch.device("cuda:0")
D, I = 3584, 18944
g = torch.Generator(device=dev).manual_seed(0)
PEAK = 8.0e12


def rnd(*s, scale=0.02):
    return torch.randn(*s, device=dev, generator=g) * scale


def w8(w, up=None):
    lin = PackedLinearW8(w, swiglu_up=up, stream_rows=128)
    lin.rows_rb = tuple(range(2, 9))   # every 17..128-row call on the FP8 streams, whatever the committed policy says
    return lin


def kinds(fn):
    ops.launch_counts_reset()
    fn()
    return {k: v for k, v in ops.launch_counts().items() if v}


def ab(name, make, ncp, M, bytes16, bytes8):
    res = {"bf16": [], "fp8": []}
    outs = {}
    for arm in ("bf16", "fp8"):
        print(f"{name:14s} M={M:3d}  {arm} launches of one call: {kinds(make(0, arm))}", flush=True)
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
    print(f"{name:14s} M={M:3d}  bf16 {fmt(res['bf16'])} us ({bytes16 / 1e6:.0f} MB, {bytes16 / t16 / 1e6:4.2f} TB/s)  "
          f"fp8 {fmt(res['fp8'])} us ({bytes8 / 1e6:.0f} MB, {bytes8 / t8 / 1e6:4.2f} TB/s, "
          f"{bytes8 / PEAK * 1e6 / t8:4.2f} of the {bytes8 / PEAK * 1e6:.1f} us floor)  fp8/bf16 {t8 / t16:.3f}  "
          f"bf16 spread {spread:.3f}  rel diff {err:.2e}  "
          f"{'WINS' if max(res['fp8']) < t16 * (1 - spread) else 'stays on the image'}", flush=True)


NG, ND = 4, 6   # copies: FP8 codes 4 x 136 MB / 6 x 68 MB, bf16 images twice that
gus = [w8(rnd(I, D).to(torch.bfloat16), rnd(I, D).to(torch.bfloat16)) for _ in range(NG)]
downs = [w8(rnd(D, I).to(torch.bfloat16)) for _ in range(ND)]
stats = ops.RowStats(128, dev)
for M in ([int(v) for v in sys.argv[1:]] or [80, 96, 112, 128]):
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
    st = [ops.RowStats(128, dev) for _ in range(ND)]
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
