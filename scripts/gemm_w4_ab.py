"""A/B of the <= 16-row MXFP4 weight stream (fo_gemm_w4, ops.PackedLinearW4) against the bf16 arm on the same model
(the existing <= 16-row kernels on the exact bf16 image of the MXFP4 weights, PackedLinearW4.bf16 -- what a bf16 engine
on the same W' runs) on the Qwen2 MLP shapes at M = 1, 8 and 16: gate/up (N 18,944, K 3,584; SwiGLU + RMSNorm consumer)
and down (N 3,584, K 18,944; + residual + next-norm statistics).  The FP8 stream (fo_gemm_w8) on weights of the same
shapes is printed beside them for information.  The method is scripts/gemm_w8_rows_ab.py's: per-launch device time from
one replayed hipGraph of launches that walk weight copies larger than the 256 MB Infinity Cache in every arm, the arms
alternated in one process, three repeats each so the spread shows, and an output check of MXFP4 against its image.
ops.W4_POLICY's rule: a GEMM streams the codes only if, at both 8 and 16 rows, its median beats the bf16 arm's median by
more than that arm's repeat-to-repeat spread; the last lines say so.
python scripts/gemm_w4_ab.py [--only gate_up|down] [rows ...] (GPU only; FO_W4_XS=7 in the environment runs the gate/up
on 7 waves x 4 code steps instead of 14 x 2)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_graph_sweep_util import graph_time  # noqa: E402
from fo import ops  # noqa: E402
from fo.ops import PackedLinearW4, PackedLinearW8  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=("gate_up", "down"), default=None)
ap.add_argument("rows", type=int, nargs="*")
args = ap.parse_args()
dev = torch.device("cuda:0")
D, I = 3584, 18944
g = torch.Generator(device=dev).manual_seed(0)
PEAK = 8.0e12
ARMS = ("bf16", "mxfp4", "fp8")
verdict = {}


def rnd(*s, scale=0.02):
    return torch.randn(*s, device=dev, generator=g) * scale


def w4(w, up=None):
    lin = PackedLinearW4(w, swiglu_up=up)
    lin.stream = True   # on the MXFP4 stream whatever the policy says
    return lin


def kinds(fn):
    ops.launch_counts_reset()
    ops.w4_launch_counts_reset()
    fn()
    c = dict(ops.launch_counts(), **ops.w4_launch_counts())
    return {k: v for k, v in c.items() if v}


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
    err = max(float((x - y).abs().max() / (x.abs().max() + 1e-30)) for x, y in zip(outs["bf16"], outs["mxfp4"]))
    med = {a: statistics.median(res[a]) for a in ARMS}
    spread = (max(res["bf16"]) - min(res["bf16"])) / med["bf16"]
    wins = med["mxfp4"] < med["bf16"] * (1 - spread)
    fmt = lambda v: "/".join(f"{t:.1f}" for t in v)   # noqa: E731
    cell = lambda a: (f"{a} {fmt(res[a])} us ({nbytes[a] / 1e6:.0f} MB, {nbytes[a] / med[a] / 1e6:4.2f} TB/s, "   # noqa: E731
                      f"{nbytes[a] / PEAK * 1e6 / med[a]:4.2f} of the {nbytes[a] / PEAK * 1e6:.1f} us floor)")
    print(f"{name:14s} M={M:2d}  {cell('bf16')}  {cell('mxfp4')}  {cell('fp8')}  mxfp4/bf16 {med['mxfp4'] / med['bf16']:.3f}  "
          f"mxfp4/fp8 {med['mxfp4'] / med['fp8']:.3f}  bf16 spread {spread:.3f}  rel diff to the image {err:.2e}  "
          f"{'WINS' if wins else 'does not win'}", flush=True)
    verdict.setdefault(name, {})[M] = wins


NG, ND = 6, 12   # copies: MXFP4 codes + scales 6 x 72 MB / 12 x 36 MB, FP8 codes twice, bf16 images four times that
ROWS = args.rows or [1, 8, 16]
stats = ops.RowStats(16, dev)
if args.only != "down":
    gus = {"mxfp4": [w4(rnd(I, D).to(torch.bfloat16), rnd(I, D).to(torch.bfloat16)) for _ in range(NG)],
           "fp8": [PackedLinearW8(rnd(I, D).to(torch.bfloat16), swiglu_up=rnd(I, D).to(torch.bfloat16)) for _ in range(NG)]}
    gus["bf16"] = [lin.bf16 for lin in gus["mxfp4"]]
    seed = ops.PackedLinear(rnd(D, 1024).to(torch.bfloat16))
    for M in ROWS:
        yg = torch.empty(M, D, device=dev)
        # producer statistics for the gate/up consumer (a projection with stats_out)
        seed(rnd(M, 1024, scale=1.0), out=rnd(M, D, scale=1.0), residual=True, M=M,
             stats_out=stats.set(torch.ones(D, device=dev), yg))
        outs = [torch.empty(M, I, device=dev) for _ in range(NG)]

        def mk_gu(i, arm, M=M, outs=outs, yg=yg):
            lin = gus[arm][i]

            def f(check=False):
                return [lin(yg, out=outs[i], M=M, norm=(stats, 1e-6))]
            return f
        ab("gate/up+rms", mk_gu, NG, M, {"bf16": gus["mxfp4"][0].nbytes, "mxfp4": gus["mxfp4"][0].fp4_nbytes,
                                         "fp8": gus["fp8"][0].fp8_nbytes})
    del gus
    torch.cuda.empty_cache()
if args.only != "gate_up":
    downs = {"mxfp4": [w4(rnd(D, I).to(torch.bfloat16)) for _ in range(ND)],
             "fp8": [PackedLinearW8(rnd(D, I).to(torch.bfloat16)) for _ in range(ND)]}
    downs["bf16"] = [lin.bf16 for lin in downs["mxfp4"]]
    for M in ROWS:
        res0 = rnd(M, D, scale=1.0)
        xm = rnd(M, I, scale=1.0)
        ys = [res0.clone() for _ in range(ND)]
        ygs = [torch.empty(M, D, device=dev) for _ in range(ND)]
        st = [ops.RowStats(16, dev) for _ in range(ND)]
        gam = torch.rand(D, device=dev, generator=g) + 0.5

        def mk_down(i, arm, M=M, xm=xm, ys=ys, ygs=ygs, st=st, gam=gam, res0=res0):
            lin = downs[arm][i]

            def f(check=False):
                if check:
                    ys[i].copy_(res0)
                lin(xm, out=ys[i], residual=True, M=M, stats_out=st[i].set(gam, ygs[i]))
                return [ys[i], ygs[i]]
            return f
        ab("down+res+stats", mk_down, ND, M, {"bf16": downs["mxfp4"][0].nbytes, "mxfp4": downs["mxfp4"][0].fp4_nbytes,
                                              "fp8": downs["fp8"][0].fp8_nbytes})
for name, v in verdict.items():
    if 8 in v and 16 in v:
        ok = v[8] and v[16]
        print(f"{name}: {'streams the MXFP4 codes at <= 16 rows' if ok else 'runs the bf16 image at every row count'} "
              f"(wins at 8 rows: {v[8]}, at 16 rows: {v[16]})", flush=True)
