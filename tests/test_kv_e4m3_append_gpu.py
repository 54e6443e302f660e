"""The paged-KV append into an FP8 (e4m3) pool: the q|k|v projection writes its fp32 K / V into a
one-page staging cache (row t = token t) and fo_kv8_append quantises the rows into the pool's codes and scales.

The projection runs at Qwen2's real width (K = 3584, 28 / 4 heads of 128; synthetic weights and bias) at M = 8, 16
(packed X), 32 and 128 -- the four dispatch families of fo_gemm_qkv_rope_kv, pinned by the launch counters -- and
through fo_gemm_w8_qkv_rope / fo_gemm_w4_qkv_rope at M = 8; one head-dim-32 case (M = 5, K = 128) is the tiny geometry.
Token slots are scattered over shuffled pages and include a page's first and last slot.  The same call runs on an fp32
pool (pre-filled with a sentinel) and, staged, on the FP8 pool (codes pre-filled with the byte 0x55, scales with 3.0).
Afterwards the FP8 pool's codes and scales at the written slots must EQUAL fo.quant.quantize_kv_rows of the fp32 pool's
rows (torch.equal on the bytes and on the scales), every other byte and scale must still be the sentinel, and q_out
must be equal.  The bias of some kv heads is multiplied by 2^4 and of others by 2^-4, so the rows' exponents differ.
"""
import random

import pytest
import torch

from fo import ops, tables
from fo.kv import KVPool
from fo.quant import quantize_kv_rows

pytestmark = pytest.mark.gpu
D, H, KVH, HD, PS, NP = 3584, 28, 4, 128, 16, 24
SENT, CODE_SENT, SCALE_SENT = -1536.0, 0x55, 3.0
EXTRA = 3   # staging rows past T (a workspace's capacity is at least its forward's rows): never read, never stored


@pytest.fixture(scope="module")
def proj(dev):
    g = torch.Generator().manual_seed(3)
    N = (H + 2 * KVH) * HD
    w = (torch.randn(N, D, generator=g) * 0.02).to(torch.bfloat16).to(dev)
    b = torch.randn(N, generator=g) * 0.5
    # K and V bias of kv heads 0 / 1 times 2^4, of kv heads 2 / 3 times 2^-4: rows of very different magnitude
    for base in (H * HD, (H + KVH) * HD):
        b[base:base + HD] *= 16.0
        b[base + HD:base + 2 * HD] *= 16.0
        b[base + 2 * HD:base + 3 * HD] /= 16.0
        b[base + 3 * HD:base + 4 * HD] /= 16.0
    b = b.to(dev)
    cos, sin = tables.rope_tables(1e6, HD, 4096, round_fp16=True)
    with torch.cuda.stream(ops.engine_stream(dev)):
        ops.Runtime.get(dev)
    return {"bf16": ops.PackedLinear(w, b, rope_hd=HD), "w": w, "b": b, "cos": cos.to(dev), "sin": sin.to(dev)}


def _slots(M, seed, n_pages=NP):
    """M distinct token slots over the pool in a shuffled order, with page 5's first and last slot and page 0's."""
    r = random.Random(seed)
    must = [5 * PS, 5 * PS + PS - 1, 0, PS - 1]
    rest = [s for s in range(n_pages * PS) if s not in must]
    r.shuffle(rest)
    sl = (must + rest)[:M]
    r.shuffle(sl)
    return sl


def _pools(dev, kvh=KVH, hd=HD):
    p32 = KVPool(1, kvh, hd, NP, PS, dev)
    p8 = KVPool(1, kvh, hd, NP, PS, dev, dtype=torch.float8_e4m3fn)
    assert p8.k.dtype == torch.float8_e4m3fn and p8.k.shape == p32.k.shape and p8.ks.shape == p32.k.shape[:-1]
    p32.k.fill_(SENT)
    p32.v.fill_(SENT)
    for t in (p8.k, p8.v):
        t.view(torch.uint8).fill_(CODE_SENT)
    for t in (p8.ks, p8.vs):
        t.fill_(SCALE_SENT)
    return p32, p8


def _pack_x(x, xp):
    """x [M <= 16 rb, K] fp32 into ops.XPack's order ([K/32][row blocks][64 lanes][8]; lane = 16 (c / 8) + row % 16)."""
    M, K = x.shape
    rb = xp.rb
    full = torch.zeros(16 * rb, K, device=x.device)
    full[:M] = x
    hi = full.to(torch.bfloat16)
    lo = (full - hi.float()).to(torch.bfloat16)
    for src, dst in ((hi, xp.hi), (lo, xp.lo)):
        dst.copy_(src.view(rb, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).reshape(-1))


def _staged(lin, x, M, pos, slot, cos, sin, q, p8, h, kvh, hd, xpack=None):
    """The stack's FP8 path (DecoderStack.forward): the GEMM appends to the staging cache, kv8_append to the pool."""
    dev = x.device
    rows = M + EXTRA
    k8 = torch.full((1, kvh, rows, hd), float("nan"), device=dev)
    v8 = torch.full((1, kvh, rows, hd), float("nan"), device=dev)
    slot8 = torch.arange(rows, dtype=torch.int32, device=dev)
    lin.qkv_rope(x, M, pos, slot8, cos, sin, q, k8, v8, h, kvh, rows, xpack=xpack)
    ops.kv8_append(k8, v8, M, slot, p8.k[0], p8.ks[0], p8.v[0], p8.vs[0], PS)
    return k8, v8


def _check_pools(p32, p8, slots, what):
    """Codes and scales at the written slots equal the CPU model of the fp32 pool's rows; the rest is the sentinel.
    Returns the set of exponents seen."""
    sl = torch.tensor(slots, dtype=torch.long)
    written = torch.zeros(NP, PS, dtype=torch.bool)
    written[sl // PS, sl % PS] = True
    exps = set()
    for name in ("k", "v"):
        a = getattr(p32, name)[0].cpu()                           # [page][kvh][slot][hd]
        codes = getattr(p8, name)[0].view(torch.uint8).cpu()
        scales = getattr(p8, name + "s")[0].cpu()                 # [page][kvh][slot]
        rows = a[sl // PS, :, sl % PS]                            # [M][kvh][hd]
        assert int((rows == SENT).sum()) == 0 and bool(torch.isfinite(rows).all()), (what, name)
        q, e, _ = quantize_kv_rows(rows)
        got_q, got_s = codes[sl // PS, :, sl % PS], scales[sl // PS, :, sl % PS]
        want_s = torch.ldexp(torch.ones_like(got_s), e)
        m = written[:, None, :].expand_as(scales)
        print(f"[kv e4m3 append] {what} {name}: {q.numel()} codes, {int((got_q != q).sum())} differ; {e.numel()} scales, "
              f"{int((got_s != want_s).sum())} differ; exponents {sorted(set(e.flatten().tolist()))}; off the sentinel: "
              f"codes {int((codes[~m] != CODE_SENT).sum())}, scales {int((scales[~m] != SCALE_SENT).sum())}, fp32 pool "
              f"{int((a[~m] != SENT).sum())}")
        assert torch.equal(got_q, q), (what, name)
        assert torch.equal(got_s, want_s), (what, name)
        assert bool((codes[~m] == CODE_SENT).all()) and bool((scales[~m] == SCALE_SENT).all()), (what, name)
        assert bool((a[~m] == SENT).all()), (what, name)
        exps |= set(e.flatten().tolist())
    return exps


# M -> the launch counters of its dispatch family (the rest of the GEMM counters stay 0)
FAMILY = {8: dict(gemm_other=1), 16: dict(gemm_other=1, gemm_xp=1), 32: dict(gemm_mid=1, gemm_rope4=1, gemm_reduce=1),
          128: dict(gemm_rows=1, gemm_reduce=1)}


@pytest.mark.parametrize("M", [8, 16, 32, 128])
def test_qkv_projection_then_append(dev, proj, M):
    lin, cos, sin = proj["bf16"], proj["cos"], proj["sin"]
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, D, generator=g).to(dev)
    slots = _slots(M, M)
    slot = torch.tensor(slots, dtype=torch.int32).to(dev)
    pos = torch.randint(0, 4096, (M,), generator=g, dtype=torch.int32).to(dev)
    xp = None
    if M == 16:   # 9..16 rows read the packed input (the previous down projection's product in a forward)
        xp = ops.XPack(D, dev, M)
        _pack_x(x, xp)
    p32, p8 = _pools(dev)
    q32 = torch.full((M, H * HD), float("nan"), device=dev)
    q8 = torch.full((M, H * HD), float("nan"), device=dev)
    with torch.cuda.stream(ops.engine_stream(dev)):
        ops.launch_counts_reset()
        lin.qkv_rope(x, M, pos, slot, cos, sin, q32, p32.k[0], p32.v[0], H, KVH, PS, xpack=xp)
        got = {k: v for k, v in ops.launch_counts().items() if k.startswith("gemm_") and v}
        assert got == FAMILY[M], (M, got)
        ops.launch_counts_reset()
        ops.kv8_launch_counts_reset()
        k8, v8 = _staged(lin, x, M, pos, slot, cos, sin, q8, p8, H, KVH, HD, xpack=xp)
        got = {k: v for k, v in ops.launch_counts().items() if k.startswith("gemm_") and v}
        assert got == FAMILY[M], (M, got)
        assert ops.kv8_launch_counts() == {"kv8_append": 1, "kv8_attention": 0}
    torch.cuda.synchronize()
    assert not torch.isnan(q32).any() and torch.equal(q8, q32)
    # the staging rows are what the fp32 pool got; the rows past M were never written
    sl = torch.tensor(slots, dtype=torch.long, device=dev)
    assert torch.equal(k8[0, :, :M].transpose(0, 1), p32.k[0][sl // PS, :, sl % PS])
    assert torch.equal(v8[0, :, :M].transpose(0, 1), p32.v[0][sl // PS, :, sl % PS])
    assert bool(torch.isnan(k8[0, :, M:]).all()) and bool(torch.isnan(v8[0, :, M:]).all())
    exps = _check_pools(p32, p8, slots, f"M = {M}")
    assert len(exps) >= 4, exps


@pytest.mark.parametrize("fmt,entry", [("fp8", "w8_qkv_rope"), ("mxfp4", "w4_qkv_rope")])
def test_quantised_qkv_projection_then_append(dev, proj, fmt, entry):
    """fo_gemm_w8_qkv_rope / fo_gemm_w4_qkv_rope at M = 8: the code-streaming q|k|v launches write the staging cache too."""
    cos, sin = proj["cos"], proj["sin"]
    lin = ops.PackedQKVQuant(proj["w"], proj["b"], HD, fmt)
    M = 8
    assert lin.streams(M)
    g = torch.Generator().manual_seed(80)
    x = torch.randn(M, D, generator=g).to(dev)
    slots = _slots(M, 81)
    slot = torch.tensor(slots, dtype=torch.int32).to(dev)
    pos = torch.randint(0, 4096, (M,), generator=g, dtype=torch.int32).to(dev)
    p32, p8 = _pools(dev)
    q32 = torch.full((M, H * HD), float("nan"), device=dev)
    q8 = torch.full((M, H * HD), float("nan"), device=dev)
    with torch.cuda.stream(ops.engine_stream(dev)):
        ops.qkv_quant_launch_counts_reset()
        ops.kv8_launch_counts_reset()
        lin.qkv_rope(x, M, pos, slot, cos, sin, q32, p32.k[0], p32.v[0], H, KVH, PS)
        _staged(lin, x, M, pos, slot, cos, sin, q8, p8, H, KVH, HD)
        c = ops.qkv_quant_launch_counts()
        assert c[entry] == 2 and sum(c.values()) == 2, c
        assert ops.kv8_launch_counts() == {"kv8_append": 1, "kv8_attention": 0}
    torch.cuda.synchronize()
    assert not torch.isnan(q32).any() and torch.equal(q8, q32)
    exps = _check_pools(p32, p8, slots, f"{fmt} M = 8")
    assert len(exps) >= 4, exps


def test_head_dim_32_tiny_geometry(dev):
    """M = 5 rows through PackedLinear(rope_hd=32) at K = 128 (4 / 2 heads of 32): a row is 8 lanes of the wave."""
    h, kvh, hd, K, M = 4, 2, 32, 128, 5
    g = torch.Generator().manual_seed(32)
    N = (h + 2 * kvh) * hd
    w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    b = torch.randn(N, generator=g) * 0.5
    b[h * hd:h * hd + hd] *= 16.0
    b[(h + kvh) * hd + hd:] /= 16.0
    b = b.to(dev)
    cos, sin = tables.rope_tables(1e6, hd, 4096, round_fp16=True)
    cos, sin = cos.to(dev), sin.to(dev)
    with torch.cuda.stream(ops.engine_stream(dev)):
        ops.Runtime.get(dev)
    lin = ops.PackedLinear(w, b, rope_hd=hd)
    x = torch.randn(M, K, generator=g).to(dev)
    slots = _slots(M, 33)
    slot = torch.tensor(slots, dtype=torch.int32).to(dev)
    pos = torch.randint(0, 4096, (M,), generator=g, dtype=torch.int32).to(dev)
    p32, p8 = _pools(dev, kvh, hd)
    q32 = torch.full((M, h * hd), float("nan"), device=dev)
    q8 = torch.full((M, h * hd), float("nan"), device=dev)
    with torch.cuda.stream(ops.engine_stream(dev)):
        ops.kv8_launch_counts_reset()
        lin.qkv_rope(x, M, pos, slot, cos, sin, q32, p32.k[0], p32.v[0], h, kvh, PS)
        _staged(lin, x, M, pos, slot, cos, sin, q8, p8, h, kvh, hd)
        assert ops.kv8_launch_counts() == {"kv8_append": 1, "kv8_attention": 0}
    torch.cuda.synchronize()
    assert not torch.isnan(q32).any() and torch.equal(q8, q32)
    exps = _check_pools(p32, p8, slots, "hd 32, M = 5")
    assert len(exps) >= 2, exps   # (K head 0 against K head 1: 2^4 apart)
