#!/usr/bin/env python3
"""One SHA-256 per case over everything the encoder's rel-pos attention launches write: the output, both rings
afterwards, and the packed halves where a packed output is armed.

k_relpos_fused and k_relpos_chunks (csrc/fo_attn.hip, one body) are deterministic and sum in a fixed order, so two
builds of the library that compute the same thing print identical files.  Inputs are seeded and generated on the CPU.
fo_relpos_attention_fused: every case of tests/relpos_ref.SINGLE_CASES (T = 9 among them), with its ring array and
with none (slot b), with and without a packed output.  fo_relpos_attention_chunks: groups of C = 2, 4, 8 chunks at
(dk 8, h 4, cap 16 / 32) and at the real geometry (dk 64, h 16, cap 72, T 4 and 7, B 8), one group of T = 9; each from
a full ring, a short one and an empty one.

    FO_LIB_PATH=/path/to/libfo_hip.so python scripts/relpos_digest.py > digest.txt      (GPU only)
"""
import hashlib
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)                 # (oracle, for the tests' helpers)
sys.path.insert(0, os.path.join(ROOT, "freeze-omni_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import relpos_ref as rr  # noqa: E402
from fo import ops  # noqa: E402

dev = torch.device("cuda:0")
GROUPS = [(8, 4, 16, 4, 2, 3), (8, 4, 16, 4, 4, 3), (8, 4, 32, 4, 8, 3),           # dk, h, cap, T, C, B
          (64, 16, 72, 4, 2, 8), (64, 16, 72, 4, 4, 8), (64, 16, 72, 4, 8, 8),
          (64, 16, 72, 7, 2, 8), (64, 16, 72, 7, 4, 8), (64, 16, 72, 7, 8, 8), (64, 2, 72, 9, 2, 2)]


def sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def ints(v):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def fused(case):
    data = case.build()
    B, T, d, cap = case.B, case.T, case.d, case.cap
    n = B * T
    for ring in ((True, False) if data.ring is not None else (False,)):
        for pack in (False, True):
            kr, vr = data.kr.to(dev), data.vr.to(dev)
            qkv = torch.zeros(n, case.ldq).to(dev)
            qkv[:, :3 * d] = data.qkv.to(dev)
            out = torch.zeros(n, case.ldo, device=dev)
            rb = (n + 15) // 16
            xp = NS(hi=torch.zeros(d * 16 * rb, dtype=torch.bfloat16, device=dev),
                    lo=torch.zeros(d * 16 * rb, dtype=torch.bfloat16, device=dev), K=d, rb=rb) if pack else None
            ops.relpos_attention_fused(qkv[:, :3 * d], kr, vr, cap, ints(case.start), ints(case.lens),
                                       ints(data.ring) if ring else None, data.ptab.to(dev), ints(case.pstart),
                                       data.bu.to(dev), data.bv.to(dev), B, T, case.h, case.dk, case.scale,
                                       out[:, :d], opack=xp)
            print(f"fused {case.name} dk={case.dk} h={case.h} cap={cap} B={B} T={T} ring={int(ring)} pack={int(pack)} "
                  f"{sha(out, kr, vr, *([xp.hi, xp.lo] if pack else []))}", flush=True)


def chunks(dk, h, cap, T, C, B):
    d = h * dk
    buffersize = cap - max(8, T)     # (len + T <= cap)
    g = torch.Generator().manual_seed(dk * 1000 + cap * 10 + C)
    slots = B + 2
    for L0 in (buffersize, 5, 0):
        kr, vr = torch.randn(slots, cap, d, generator=g).to(dev), torch.randn(slots, cap, d, generator=g).to(dev)
        qkv = torch.randn(C * B * T, 3 * d, generator=g).to(dev)
        ptab = torch.randn(600, d, generator=g).to(dev)
        bu, bv = torch.randn(d, generator=g).to(dev), torch.randn(d, generator=g).to(dev)
        starts = [(3 * b + 1) % cap for b in range(B)]
        lens = [min(L0, buffersize)] * B
        rings = [slots - 1 - b for b in range(B)]
        pe = [40 + 4 * b for b in range(B)]
        metas = []
        for _ in range(C):      # the ring bookkeeping of C sequential chunks (SpeechEncoderEngine.advance's rule)
            metas.append(starts + lens + rings + [max(0, p - 3 * T) for p in pe])
            for b in range(B):
                total = lens[b] + T
                keep = min(total, buffersize)
                starts[b] = (starts[b] + total - keep) % cap
                lens[b] = keep
                pe[b] += T
        out = torch.zeros(C * B * T, d, device=dev)
        ops.relpos_attention_chunks(qkv, kr, vr, cap, ints(np.concatenate(metas)), B, C, ptab, bu, bv, T, h, dk,
                                    1.0 / math.sqrt(dk), out)
        print(f"chunks dk={dk} h={h} cap={cap} B={B} T={T} C={C} L0={min(L0, buffersize)} {sha(out, kr, vr)}",
              flush=True)


def main():
    for case in rr.SINGLE_CASES:
        fused(case)
    for grp in GROUPS:
        chunks(*grp)


if __name__ == "__main__":
    main()
