#!/usr/bin/env python3
"""A/B of the encoder's rel-pos attention kernels (k_relpos_fused, k_relpos_chunks) between two builds of the library.

Per-launch device time from a replayed hipGraph (gemm_graph_sweep_util.graph_time) at the real geometry: the heads,
head size, chunk and ring capacity SpeechEncoderEngine computes for configs/real.
  k_relpos_fused   B = 1, 2, 8 users x T = 4 frames, from a full ring and from an empty one, with and without the
                   packed output
  k_relpos_chunks  B = 8 users x C = 2 and 8 chunks of 4 frames from a full ring (the time includes
                   k_relpos_chunks_append, the entry's second launch, the same code in both builds)

    python scripts/relpos_ab.py                      one library (FO_LIB_PATH): three repeats per cell   (GPU only)
    python scripts/relpos_ab.py --ab PARENT NEW > profiles/relpos_fold_ab.txt

--ab runs the libraries parent / new / parent / new, each in a process of its own, and applies DESIGN 5.5's rule: per
cell the new median over its 6 figures may exceed the parent's median by no more than the parent's own spread at that
cell (max - min of its 6 figures).  Exit 1 if a cell is over.
"""
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REPS, REPEATS = 200, 3


def cells():
    import torch
    import yaml

    from gemm_graph_sweep_util import graph_time
    from fo import ops
    from fo.speech import ring_geometry
    from types import SimpleNamespace as NS
    with open(os.path.join(ROOT, "configs", "real", "audiollm", "train.yaml")) as f:
        tr = yaml.safe_load(f)["encoder_conf"]["para_conf"]["transformer"]
    d, h, T = tr["transformer-attention-dim"], tr["transformer-attention-heads"], tr["transformer-chunk_size"]
    buffersize, _, _, cap = ring_geometry(T, tr["transformer-left_chunks"])
    dk = d // h
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    def ints(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)

    def meta(B, C, L0):
        """start B | len B | ring B | pstart B per chunk, by SpeechEncoderEngine.advance's rule"""
        starts, lens, pe, out = [(5 * b + 3) % cap for b in range(B)], [L0] * B, [400 + 4 * b for b in range(B)], []
        for _ in range(C):
            out += starts + lens + list(range(B)) + [p - buffersize - T for p in pe]
            for b in range(B):
                keep = min(lens[b] + T, buffersize)
                starts[b] = (starts[b] + lens[b] + T - keep) % cap
                lens[b] = keep
                pe[b] += T
        return ints(out)

    ptab, bu, bv = rnd(1000, d), rnd(d), rnd(d)
    scale = 1.0 / math.sqrt(dk)
    for B in (1, 2, 8):
        for L0 in (buffersize, 0):
            for pack in (0, 1):
                kr, vr, qkv, out = rnd(B, cap, d), rnd(B, cap, d), rnd(B * T, 3 * d), torch.zeros(B * T, d, device=dev)
                m = meta(B, 1, L0)
                rb = (B * T + 15) // 16
                xp = NS(hi=torch.zeros(d * 16 * rb, dtype=torch.bfloat16, device=dev),
                        lo=torch.zeros(d * 16 * rb, dtype=torch.bfloat16, device=dev), K=d, rb=rb) if pack else None
                yield (f"fused B={B} T={T} ring={'full' if L0 else 'empty'} pack={pack}",
                       lambda: ops.relpos_attention_fused(qkv, kr, vr, cap, m[:B], m[B:2 * B], m[2 * B:3 * B], ptab,
                                                          m[3 * B:], bu, bv, B, T, h, dk, scale, out, opack=xp),
                       graph_time)
    for C in (2, 8):
        B = 8
        kr, vr, qkv, out = rnd(B, cap, d), rnd(B, cap, d), rnd(C * B * T, 3 * d), torch.zeros(C * B * T, d, device=dev)
        m = meta(B, C, buffersize)
        yield (f"chunks B={B} T={T} C={C} ring=full",
               lambda: ops.relpos_attention_chunks(qkv, kr, vr, cap, m, B, C, ptab, bu, bv, T, h, dk, scale, out),
               graph_time)


def one():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    for name, fn, graph_time in cells():
        print("%s | %s" % (name, " ".join("%.2f" % graph_time(fn, REPS) for _ in range(REPEATS))), flush=True)


def ab(parent, new):
    figs = {}
    for arm, lib in (("parent", parent), ("new", new)) * 2:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, FO_LIB_PATH=lib),
                           capture_output=True, text=True, timeout=300)
        if p.returncode:
            sys.exit("%s run failed (%d):\n%s" % (arm, p.returncode, p.stderr[-2000:]))
        for line in p.stdout.splitlines():
            name, vals = line.split(" | ")
            figs.setdefault(name, {"parent": [], "new": []})[arm] += [float(v) for v in vals.split()]
    print(__doc__.split("\n\n")[1])
    print("Per-launch us over %d replayed launches; %d repeats a run, runs parent / new / parent / new, a process each."
          % (REPS, REPEATS))
    print("Rule: the new median over its 6 figures may exceed the parent's by no more than the parent's own spread "
          "(max - min of its 6 figures).\n")
    print("cell: parent repeats (both runs) | new repeats (both runs) | medians parent > new, parent spread, verdict")
    over = 0
    for name, f in figs.items():
        mp, mn = statistics.median(f["parent"]), statistics.median(f["new"])
        spread = max(f["parent"]) - min(f["parent"])
        ok = mn - mp <= spread + 1e-9
        over += not ok
        print("%s: %s | %s | %.3f > %.3f us (%+.3f), spread %.2f: %s"
              % (name, "/".join("%.2f" % v for v in f["parent"]), "/".join("%.2f" % v for v in f["new"]), mp, mn,
                 mn - mp, spread, "within" if ok else "OVER"))
    print("\n%d cells, %d over the rule" % (len(figs), over))
    return 1 if over else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--ab":
        sys.exit(ab(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3])))
    one()
