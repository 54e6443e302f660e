#!/usr/bin/env python3
"""One SHA-256 per (format, entry, case) over the output bytes of every quantised weight-stream GEMM entry.

Every form of these kernels is deterministic and sums in a fixed order, so two builds of the library that compute the
same thing print identical files.  Inputs are seeded and generated on the CPU; the weights are quantised by the
library's own quantisers; the entries are called through the C-ABI with this script's own workspace and tickets (left
zeroed: checked).  The cases are the smallest that reach every kernel instantiation and every edge the kernels handle
(K % 128 and K % 64 tails, a partial last tile, an odd tile count, split and unsplit K, the FO_W*_XS shapes in a child
process).

    FO_LIB_PATH=/path/to/libfo_hip.so python scripts/gemm_wq_digest.py > digest.txt      (GPU only)
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "freeze-omni_amd"))
from fo import _lib, ops  # noqa: E402

dev = torch.device("cuda:0")
FMTS = {"fp8": ("w8", "FO_W8_XS", "8"), "mxfp4": ("w4", "FO_W4_XS", "7"), "mxfp6": ("w6", "FO_W6_XS", "7")}
WS = torch.zeros(1 << 21, device=dev)
TICKETS = torch.zeros(4096, dtype=torch.int32, device=dev)
seed = [0]


def rnd(*shape, scale=1.0, pos=False):
    seed[0] += 1
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed[0])) * scale
    return (t.abs() + 0.5 if pos else t).to(dev)


def sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def codes(fmt, N, K, swiglu):
    """Packed codes and scales of a seeded [N, K] weight (SwiGLU: the gate and the up, interleaved tiles)."""
    fm = ops.QUANT_FORMATS[fmt]
    nt = (N + 15) // 16 * (2 if swiglu else 1)
    q, sc = ops._code_storage(fm, nt, K, dev)
    for base in range(2 if swiglu else 1):
        ops._quant_codes(fmt, rnd(N, K, scale=0.05), q, sc, base, 2 if swiglu else 1)
    return q, sc, nt


def mlp(fmt, entry, case, M, K, N, swiglu, residual=False, rstats=False, producer=False, ws=True):
    q, sc, nt = codes(fmt, N, K, swiglu)
    x, y = rnd(M, K), rnd(M, N)
    units = (N + 15) // 16
    st = rnd(M, 3, pos=True) if rstats else None
    so, gn, yg = (torch.zeros(M, units, device=dev), rnd(N), torch.zeros(M, N, device=dev)) if producer else (None,) * 3
    sg = ctypes.c_int(0)
    p = ops.ptr
    _lib.call(entry, x.data_ptr(), K, M, K, q.data_ptr(), sc.data_ptr(), nt, N, int(swiglu), y.data_ptr(), N,
              int(residual), WS.data_ptr() if ws else None, WS.numel() if ws else 0, TICKETS.data_ptr() if ws else None,
              p(st), 3 if rstats else 0, 1e-6, p(so), p(gn), p(yg), ctypes.byref(sg), ops.stream(dev))
    outs = [y] + ([so, yg] if producer else [])
    print(f"{fmt} {entry} {case} M={M} K={K} N={N} {sha(*outs)}", flush=True)
    assert int(TICKETS.abs().sum()) == 0, "tickets not left zeroed"


def general(fmt, w):
    for K in ((96, 1056, 2144) if fmt == "fp8" else (160, 2144)):
        for M in (1, 5, 16):
            mlp(fmt, f"fo_gemm_{w}", "swiglu", M, K, 40, True)
            mlp(fmt, f"fo_gemm_{w}", "swiglu+rstats", M, K, 40, True, rstats=True)
            mlp(fmt, f"fo_gemm_{w}", "plain", M, K, 40, False)
            mlp(fmt, f"fo_gemm_{w}", "plain+rstats", M, K, 40, False, rstats=True)
            mlp(fmt, f"fo_gemm_{w}", "plain+residual", M, K, 40, False, residual=True)
            mlp(fmt, f"fo_gemm_{w}", "plain+producer", M, K, 40, False, residual=True, producer=True)


def xs(fmt, w, tag="xs"):
    for M in (1, 16):
        mlp(fmt, f"fo_gemm_{w}", tag, M, 3584, 48, True, rstats=True)


def head(fmt, w):
    q, sc, nt = codes(fmt, 40, 3584, False)
    x, y = rnd(3, 3584), rnd(3, 40)
    _lib.call(f"fo_gemm_{w}_head", x.data_ptr(), 3584, 3, 3584, q.data_ptr(), sc.data_ptr(), nt, 40, y.data_ptr(), 40,
              ops.stream(dev))
    print(f"{fmt} fo_gemm_{w}_head head M=3 K=3584 N=40 {sha(y)}", flush=True)


def sk(fmt, w):
    for K in ((4096, 8192) if fmt == "fp8" else (8192,)):   # (e4m3 splits from 128 code steps: K = 8192)
        for M in (1, 16):
            mlp(fmt, f"fo_gemm_{w}", "sk", M, K, 256, False, residual=True, producer=True)
    mlp(fmt, f"fo_gemm_{w}", "sk-no-workspace", 16, 8192, 256, False, ws=False)


def qkv(fmt, w):
    hd, H, KVH, PS = 64, 2, 1, 16
    N = (H + 2 * KVH) * hd
    fm = ops.QUANT_FORMATS[fmt]
    for K in (160, 2048):
        q, sc = ops._code_storage(fm, N // 16, K, dev)
        wt = rnd(N, K, scale=0.05)
        for h in range(N // hd):
            for p in (0, 1):
                r0 = h * hd + p * (hd // 2)
                ops._quant_codes(fmt, wt[r0:r0 + hd // 2], q, sc, h * (hd // 16) + p, 2)
        for M in (1, 16):
            for cdt in (torch.float32, torch.bfloat16):
                x, bias, st = rnd(M, K), rnd(N), rnd(M, 3, pos=True)
                pos = torch.arange(M, dtype=torch.int32, device=dev) * 3 + 1
                slot = torch.arange(M, dtype=torch.int32, device=dev) * 2 + 1
                cos_t, sin_t = rnd(64, hd // 2), rnd(64, hd // 2)
                q_out = rnd(M, H * hd)
                kc, vc = rnd(3, KVH, PS, hd).to(cdt), rnd(3, KVH, PS, hd).to(cdt)
                _lib.call(f"fo_gemm_{w}_qkv_rope", x.data_ptr(), K, M, K, q.data_ptr(), sc.data_ptr(), N // 16, N,
                          bias.data_ptr(), st.data_ptr(), 3, 1e-6, pos.data_ptr(), slot.data_ptr(), cos_t.data_ptr(),
                          sin_t.data_ptr(), q_out.data_ptr(), kc.data_ptr(), vc.data_ptr(), H, KVH, hd, PS,
                          4 if cdt == torch.float32 else 2, ops.stream(dev))
                print(f"{fmt} fo_gemm_{w}_qkv_rope {'fp32' if cdt == torch.float32 else 'bf16'}-cache M={M} K={K} "
                      f"{sha(q_out, kc, vc)}", flush=True)


def rows(fmt, w):
    for M in (17, 40, 64):
        for K in (864, 3584):
            mlp(fmt, f"fo_gemm_{w}_rows", "swiglu+rstats", M, K, 48, True, rstats=True)
            mlp(fmt, f"fo_gemm_{w}_rows", "plain+producer", M, K, 40, False, residual=True, producer=True)
    if fmt == "fp8":
        for M in (65, 128):
            mlp(fmt, "fo_gemm_w8_rows128", "swiglu+rstats", M, 864, 48, True, rstats=True)
            mlp(fmt, "fo_gemm_w8_rows128", "plain+producer", M, 864, 40, False, residual=True, producer=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--xs-alt":   # the child: one format's A/B xs shape
        fmt = sys.argv[2]
        seed[0] = 1 << 20
        return xs(fmt, FMTS[fmt][0], "xs-alt")
    for fmt, (w, env, val) in FMTS.items():
        general(fmt, w)
        xs(fmt, w)
        head(fmt, w)
        sk(fmt, w)
        if ops.QUANT_FORMATS[fmt].qkv_rope:
            qkv(fmt, w)
        rows(fmt, w)
        torch.cuda.synchronize()
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.abspath(__file__), "--xs-alt", fmt], env=dict(os.environ, **{env: val}),
                       check=True, timeout=120)


if __name__ == "__main__":
    main()
