"""A/B of the quantised Qwen2 output head at <= 16 rows: the FP8 stream (fo_gemm_w8_head) and the MXFP4 stream
(fo_gemm_w4_head) against the bf16 arm -- the exact bf16 image of the FP8 head's W' on the head's existing kernel,
what lm_head_weights="bf16" runs -- at N = 152,064, K = 3,584 and M = 1, 8 and 16.  The method is scripts/gemm_w4_ab.py's:
per-launch device time from one replayed hipGraph of launches that walk weight copies larger than the 256 MB Infinity
Cache in every arm (two copies per format: 2 x 290 MB of MXFP4 codes and scales, 2 x 545 MB of FP8 codes, 2 x 1.09 GB of
image), the arms alternated in one process, three repeats each so the spread shows, and an output check of each stream
against its own image.  ops.HEAD_POLICY's rule (DESIGN 5.5's): a format streams its codes only if, at both 8 and 16
rows, its median beats the bf16 arm's median by more than that arm's repeat-to-repeat spread (max - min); the last lines
say so.
python scripts/gemm_head_ab.py [rows ...] (GPU only)"""
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
ap.add_argument("rows", type=int, nargs="*")
args = ap.parse_args()
dev = torch.device("cuda:0")
V, D = 152064, 3584
NCP = 2
g = torch.Generator(device=dev).manual_seed(0)
PEAK = 8.0e12
ARMS = ("bf16", "fp8", "mxfp4")
verdict = {a: {} for a in ARMS[1:]}


def rnd(*s, scale=0.02):
    return torch.randn(*s, device=dev, generator=g) * scale


def head(cls):
    lin = cls(rnd(V, D).to(torch.bfloat16), kind="head")
    lin.stream = True   # on the stream whatever the policy says
    torch.cuda.empty_cache()
    return lin


def kinds(fn):
    ops.launch_counts_reset()
    ops.w4_launch_counts_reset()
    ops.head_launch_counts_reset()
    fn()
    c = dict(ops.launch_counts(), **ops.w4_launch_counts(), **ops.head_launch_counts())
    return {k: v for k, v in c.items() if v}


heads = {"fp8": [head(PackedLinearW8) for _ in range(NCP)], "mxfp4": [head(PackedLinearW4) for _ in range(NCP)]}
lins = dict(heads, bf16=[lin.bf16 for lin in heads["fp8"]])
nbytes = {"bf16": lins["bf16"][0].nbytes, "fp8": heads["fp8"][0].fp8_nbytes, "mxfp4": heads["mxfp4"][0].fp4_nbytes}
print(f"lm_head {V} x {D}: bf16 image {nbytes['bf16'] / 1e6:.1f} MB, FP8 codes + scales {nbytes['fp8'] / 1e6:.1f} MB, "
      f"MXFP4 codes + scales {nbytes['mxfp4'] / 1e6:.1f} MB; {NCP} cold copies per arm", flush=True)
for M in args.rows or [1, 8, 16]:
    x = rnd(M, D, scale=1.0)
    outs = [torch.empty(M, V, device=dev) for _ in range(NCP)]

    def make(i, arm, M=M, x=x, outs=outs):
        return lambda: lins[arm][i](x, out=outs[i], M=M)
    res = {a: [] for a in ARMS}
    for arm in ARMS:
        print(f"lm_head M={M:2d}  {arm} launches of one call: {kinds(make(0, arm))}", flush=True)
    for _ in range(3):
        for arm in ARMS:
            fns = [make(i, arm) for i in range(NCP)]
            it = iter(range(1 << 30))
            res[arm].append(graph_time(lambda: fns[next(it) % NCP](), NCP * 12))
    err = {}
    for arm in ARMS[1:]:   # each stream against its own image
        y = heads[arm][0](x, M=M)
        ref = heads[arm][0].bf16(x, M=M)
        torch.cuda.synchronize()
        err[arm] = float((y - ref).abs().max() / ref.abs().max())
    med = {a: statistics.median(res[a]) for a in ARMS}
    spread = max(res["bf16"]) - min(res["bf16"])
    fmt = lambda v: "/".join(f"{t:.1f}" for t in v)   # noqa: E731
    cell = lambda a: (f"{a} {fmt(res[a])} us ({nbytes[a] / med[a] / 1e6:4.2f} TB/s, "   # noqa: E731
                      f"{nbytes[a] / PEAK * 1e6 / med[a]:4.2f} of the {nbytes[a] / PEAK * 1e6:.1f} us floor)")
    line = f"lm_head M={M:2d}  {cell('bf16')}  {cell('fp8')}  {cell('mxfp4')}  bf16 spread {spread:.1f} us"
    for arm in ARMS[1:]:
        wins = med[arm] < med["bf16"] - spread
        verdict[arm][M] = wins
        line += (f"  {arm}/bf16 {med[arm] / med['bf16']:.3f} ({'WINS' if wins else 'does not win'}, rel diff to its image "
                 f"{err[arm]:.2e})")
    print(line, flush=True)
for arm, v in verdict.items():
    if 8 in v and 16 in v:
        ok = v[8] and v[16]
        print(f"{arm}: HEAD_POLICY {ok} -- {'streams the codes at <= 16 rows' if ok else 'runs the bf16 image at every row count'} "
              f"(wins at 8 rows: {v[8]}, at 16 rows: {v[16]})", flush=True)
