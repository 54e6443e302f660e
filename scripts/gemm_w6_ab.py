"""A/B of the <= 16-row MXFP6 weight stream (fo_gemm_w6 / fo_gemm_w6_head, ops.PackedLinearW6) on the three Qwen2 GEMMs
it serves, at M = 1, 8 and 16: gate/up (N 18,944, K 3,584; SwiGLU + RMSNorm consumer), down (N 3,584, K 18,944;
+ residual + next-norm statistics) and the output head (N 152,064, K 3,584; plain).  Four arms: the bf16 arm on the same
model (the existing <= 16-row kernels on the exact bf16 image of the MXFP6 weights, PackedLinearW6.bf16 -- what a bf16
engine on the same W' runs), the FP8 stream, the MXFP6 stream and the MXFP4 stream on weights of the same shapes.  The
method is scripts/gemm_w4_ab.py's: per-launch device time from one replayed hipGraph of launches that walk weight copies
larger than the 256 MB Infinity Cache in every arm, the arms alternated in one process, three repeats each so the
spread shows, and an output check of MXFP6 against its image.
ops.W6_POLICY's rule (DESIGN 5.5's): a GEMM streams the MXFP6 codes only if, at both 8 and 16 rows, its median beats the
bf16 arm's median by more than that arm's repeat-to-repeat spread (max - min); the last lines say so, and say per GEMM
whether the MXFP6 stream beat the FP8 stream of the same process and by how much.
python scripts/gemm_w6_ab.py [--only gate_up|down|head] [rows ...] (GPU only; FO_W6_XS=7 in the environment runs the
gate/up on 7 waves x 4 code steps instead of 14 x 2)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_graph_sweep_util import graph_time  # noqa: E402
from fo import ops  # noqa: E402
from fo.ops import PackedLinearW4, PackedLinearW6, PackedLinearW8  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=("gate_up", "down", "head"), default=None)
ap.add_argument("rows", type=int, nargs="*")
args = ap.parse_args()
dev = torch.device("cuda:0")
D, I, V = 3584, 18944, 152064
g = torch.Generator(device=dev).manual_seed(0)
PEAK = 8.0e12
ARMS = ("bf16", "fp8", "mxfp6", "mxfp4")
CLS = {"fp8": PackedLinearW8, "mxfp6": PackedLinearW6, "mxfp4": PackedLinearW4}
CODES = {"fp8": "fp8_nbytes", "mxfp6": "fp6_nbytes", "mxfp4": "fp4_nbytes"}
verdict, vs_fp8 = {}, {}


def rnd(*s, scale=0.02):
    return torch.randn(*s, device=dev, generator=g) * scale


def lin_of(arm, w, up=None, kind=None):
    lin = CLS[arm](w, swiglu_up=up, kind=kind)
    lin.stream = True   # on the code stream whatever the policy says
    return lin


def family(n, shape, swiglu=False, kind=None):
    """n cold copies per format; the bf16 arm is the image of the MXFP6 copies."""
    fam = {a: [lin_of(a, rnd(*shape).to(torch.bfloat16), rnd(*shape).to(torch.bfloat16) if swiglu else None, kind)
               for _ in range(n)] for a in ARMS[1:]}
    fam["bf16"] = [lin.bf16 for lin in fam["mxfp6"]]
    torch.cuda.empty_cache()
    nbytes = {a: getattr(fam[a][0], CODES[a]) for a in ARMS[1:]}
    nbytes["bf16"] = fam["mxfp6"][0].nbytes
    return fam, nbytes


def kinds(fn):
    ops.launch_counts_reset()
    ops.w4_launch_counts_reset()
    ops.w6_launch_counts_reset()
    ops.head_launch_counts_reset()
    fn()
    c = dict(ops.launch_counts(), **ops.w4_launch_counts(), **ops.w6_launch_counts(), **ops.head_launch_counts())
    return {k: v for k, v in c.items() if v}


def ab(name, make, ncp, M, nbytes, reps):
    res = {a: [] for a in ARMS}
    outs = {}
    for arm in ARMS:
        print(f"{name:14s} M={M:2d}  {arm} launches of one call: {kinds(make(0, arm))}", flush=True)
    for _ in range(3):
        for arm in ARMS:
            fns = [make(i, arm) for i in range(ncp)]
            it = iter(range(1 << 30))
            res[arm].append(graph_time(lambda: fns[next(it) % ncp](), reps))
            if arm in ("bf16", "mxfp6"):
                o = fns[0](check=True)
                torch.cuda.synchronize()
                outs[arm] = [t.clone() for t in o]
    err = max(float((x - y).abs().max() / (x.abs().max() + 1e-30)) for x, y in zip(outs["bf16"], outs["mxfp6"]))
    med = {a: statistics.median(res[a]) for a in ARMS}
    spread = max(res["bf16"]) - min(res["bf16"])
    wins = med["mxfp6"] < med["bf16"] - spread
    fmt = lambda v: "/".join(f"{t:.1f}" for t in v)   # noqa: E731
    cell = lambda a: (f"{a} {fmt(res[a])} us ({nbytes[a] / 1e6:.0f} MB, {nbytes[a] / med[a] / 1e6:4.2f} TB/s, "   # noqa: E731
                      f"{nbytes[a] / PEAK * 1e6 / med[a]:4.2f} of the {nbytes[a] / PEAK * 1e6:.1f} us floor)")
    print(f"{name:14s} M={M:2d}  " + "  ".join(cell(a) for a in ARMS) +
          f"  mxfp6/bf16 {med['mxfp6'] / med['bf16']:.3f}  mxfp6/fp8 {med['mxfp6'] / med['fp8']:.3f}  "
          f"mxfp4/mxfp6 {med['mxfp4'] / med['mxfp6']:.3f}  bf16 spread {spread:.1f} us  rel diff to the image {err:.2e}  "
          f"{'WINS' if wins else 'does not win'}", flush=True)
    verdict.setdefault(name, {})[M] = wins
    vs_fp8.setdefault(name, {})[M] = (med["mxfp6"], med["fp8"], max(res["fp8"]) - min(res["fp8"]))


NG, ND, NH = 6, 12, 2   # copies: MXFP6 codes + scales 6 x 106 MB / 12 x 53 MB / 2 x 426 MB; MXFP4 fewer bytes still > 256 MB
ROWS = args.rows or [1, 8, 16]
stats = ops.RowStats(16, dev)
if args.only in (None, "gate_up"):
    gus, nb = family(NG, (I, D), swiglu=True)
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
        ab("gate/up+rms", mk_gu, NG, M, nb, 48)
    del gus
    torch.cuda.empty_cache()
if args.only in (None, "down"):
    downs, nb = family(ND, (D, I))
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
        ab("down+res+stats", mk_down, ND, M, nb, 48)
    del downs
    torch.cuda.empty_cache()
if args.only in (None, "head"):
    heads, nb = family(NH, (V, D), kind="head")
    for M in ROWS:
        x = rnd(M, D, scale=1.0)
        outs = [torch.empty(M, V, device=dev) for _ in range(NH)]

        def mk_head(i, arm, M=M, x=x, outs=outs):
            lin = heads[arm][i]

            def f(check=False):
                return [lin(x, out=outs[i], M=M)]
            return f
        ab("lm_head", mk_head, NH, M, nb, NH * 12)
for name, v in verdict.items():
    if 8 in v and 16 in v:
        ok = v[8] and v[16]
        print(f"{name}: W6_POLICY {ok} -- {'streams the MXFP6 codes at <= 16 rows' if ok else 'runs the bf16 image at every row count'} "
              f"(wins at 8 rows: {v[8]}, at 16 rows: {v[16]})", flush=True)
        for M in (8, 16):
            m6, m8, sp8 = vs_fp8[name][M]
            say = "beats" if m6 < m8 - sp8 else ("is level with" if abs(m6 - m8) <= sp8 else "loses to")
            print(f"{name} M={M}: the MXFP6 stream {say} the FP8 stream: {m6:.1f} us against {m8:.1f} us "
                  f"({(m8 - m6) / m8 * 100:+.1f} % of the FP8 time; FP8 spread {sp8:.1f} us)", flush=True)
