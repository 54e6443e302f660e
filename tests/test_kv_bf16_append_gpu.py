"""The paged-KV append into a bf16 pool: the q|k|v projection's RoPE epilogues and fo_rope_kv_write store
f2bf(x) as 2-byte elements where an fp32 pool under fo_set_kv_bf16(1) stores the same bf16 value widened.

The projection runs at Qwen2's real width (K = 3584, 28 / 4 heads of 128; synthetic weights and bias) at M = 8, 16,
32 and 128 -- the four dispatch families that end in rope_store / rope_store_pre: k_gemm<2, 1, ...> (<= 8 rows),
k_gemm_xp<2, 1, 16, 4> on packed X (9..16), the 4-tile column groups + k_gemm_reduce (17..64) and k_gemm_rows + reduce
(65..128); the launch counters pin each.  Token slots are scattered over shuffled pages and include a page's first and
last slot.  Both pools start from a sentinel; afterwards pool16.float() must EQUAL the fp32 pool everywhere (written
slots: the same values; every other element: still the sentinel), and q_out must be equal.
"""
import random

import pytest
import torch

from fo import _lib, ops, tables
from fo.kv import KVPool

pytestmark = pytest.mark.gpu
D, H, KVH, HD, PS, NP = 3584, 28, 4, 128, 16, 24
SENT = -1536.0   # bf16-representable (1.5 x 2^10), far from every K / V value


@pytest.fixture(scope="module")
def proj(dev):
    g = torch.Generator().manual_seed(3)
    N = (H + 2 * KVH) * HD
    w = (torch.randn(N, D, generator=g) * 0.02).to(torch.bfloat16).to(dev)
    b = (torch.randn(N, generator=g) * 0.5).to(dev)
    cos, sin = tables.rope_tables(1e6, HD, 4096, round_fp16=True)
    with torch.cuda.stream(ops.engine_stream(dev)):
        ops.Runtime.get(dev)
    return ops.PackedLinear(w, b, rope_hd=HD), w, b, cos.to(dev), sin.to(dev)


def _slots(M, seed):
    """M distinct token slots over the pool in a shuffled order, with page 5's first and last slot and page 0's."""
    r = random.Random(seed)
    must = [5 * PS, 5 * PS + PS - 1, 0, PS - 1]
    rest = [s for s in range(NP * PS) if s not in must]
    r.shuffle(rest)
    sl = (must + rest)[:M]
    r.shuffle(sl)
    return sl


def _pools(dev):
    p32 = KVPool(1, KVH, HD, NP, PS, dev)
    p16 = KVPool(1, KVH, HD, NP, PS, dev, dtype=torch.bfloat16)
    for p in (p32, p16):
        p.k.fill_(SENT)
        p.v.fill_(SENT)
    return p32, p16


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


def _check_pools(p32, p16, slots, what):
    sl = torch.tensor(slots, dtype=torch.long, device=p32.k.device)
    written = torch.zeros(NP, PS, dtype=torch.bool, device=p32.k.device)
    written[sl // PS, sl % PS] = True
    mask = written[None, :, None, :, None].expand_as(p32.k)
    for name in ("k", "v"):
        a, b = getattr(p32, name), getattr(p16, name)
        assert b.dtype == torch.bfloat16 and a.dtype == torch.float32
        wa, wb = a[mask], b[mask].float()
        print(f"[kv bf16 append] {what} {name}: {wa.numel()} written elements, {int((wa != wb).sum())} differ; "
              f"unwritten off the sentinel: fp32 pool {int((a[~mask] != SENT).sum())}, bf16 pool "
              f"{int((b[~mask].float() != SENT).sum())}")
        assert torch.equal(wb, wa), (what, name)
        assert torch.equal(wa, wa.to(torch.bfloat16).float()), (what, name)   # the fp32 pool holds bf16 values
        assert int((wa == SENT).sum()) == 0 and float(wa.abs().max()) < 100.0, (what, name)
        assert bool((a[~mask] == SENT).all()) and bool((b[~mask].float() == SENT).all()), (what, name)


# M -> the launch counters of its dispatch family (the rest of the GEMM counters stay 0)
FAMILY = {8: dict(gemm_other=1), 16: dict(gemm_other=1, gemm_xp=1), 32: dict(gemm_mid=1, gemm_rope4=1, gemm_reduce=1),
          128: dict(gemm_rows=1, gemm_reduce=1)}


@pytest.mark.parametrize("M", [8, 16, 32, 128])
def test_qkv_projection_appends_the_same_values(dev, proj, M):
    lin, w, b, cos, sin = proj
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, D, generator=g).to(dev)
    slots = _slots(M, M)
    slot = torch.tensor(slots, dtype=torch.int32).to(dev)
    pos = torch.randint(0, 4096, (M,), generator=g, dtype=torch.int32).to(dev)
    xp = None
    if M == 16:   # 9..16 rows read the packed input (the previous down projection's product in a forward)
        xp = ops.XPack(D, dev, M)
        _pack_x(x, xp)
    p32, p16 = _pools(dev)
    qs = []
    lib = _lib.load()
    prev = lib.fo_set_kv_bf16(1)
    assert prev in (0, 1)
    try:
        with torch.cuda.stream(ops.engine_stream(dev)):
            for pool in (p32, p16):
                q = torch.full((M, H * HD), float("nan"), device=dev)
                ops.launch_counts_reset()
                lin.qkv_rope(x, M, pos, slot, cos, sin, q, pool.k[0], pool.v[0], H, KVH, PS, xpack=xp)
                c = ops.launch_counts()
                want = FAMILY[M]
                got = {k: v for k, v in c.items() if k.startswith("gemm_") and v}
                assert got == want, (M, got, want)
                qs.append(q)
        torch.cuda.synchronize()
    finally:
        assert lib.fo_set_kv_bf16(prev) == 1
    assert not torch.isnan(qs[0]).any() and torch.equal(qs[0], qs[1])
    _check_pools(p32, p16, slots, f"M = {M}")
    # V has no rotation: the appended rows are the bf16 rounding of x Wv^T + b (float64 here; an element may land on
    # the neighbouring bf16 value, 2^-8 relative, where the fp32 sum sits at a rounding boundary)
    sl = torch.tensor(slots, dtype=torch.long, device=dev)
    wv, bv = w[(H + KVH) * HD:].double(), b[(H + KVH) * HD:].double()
    ref = (x.double() @ wv.T + bv).view(M, KVH, HD)
    got = p16.v[0][sl // PS, :, sl % PS].double()
    torch.testing.assert_close(got, ref, rtol=2 ** -7, atol=1e-3)


def test_rope_kv_write_appends_the_same_values(dev, proj):
    """fo_rope_kv_write on one 5-row q|k|v: the same equalities (an fp32 pool's appended rows are rounded to bf16
    values under fo_set_kv_bf16(1) here too)."""
    _, _, _, cos, sin = proj
    T = 5
    g = torch.Generator().manual_seed(55)
    qkv = torch.randn(T, (H + 2 * KVH) * HD, generator=g).to(dev)
    slots = _slots(T, 55)
    slot = torch.tensor(slots, dtype=torch.int32).to(dev)
    pos = torch.randint(0, 4096, (T,), generator=g, dtype=torch.int32).to(dev)
    p32, p16 = _pools(dev)
    qs = []
    lib = _lib.load()
    prev = lib.fo_set_kv_bf16(1)
    try:
        for pool in (p32, p16):
            q = torch.full((T, H * HD), float("nan"), device=dev)
            ops.rope_kv_write(qkv, T, H, KVH, HD, pos, slot, cos, sin, q, pool.k[0], pool.v[0], PS)
            qs.append(q)
        torch.cuda.synchronize()
    finally:
        assert lib.fo_set_kv_bf16(prev) == 1
    assert not torch.isnan(qs[0]).any() and torch.equal(qs[0], qs[1])
    _check_pools(p32, p16, slots, "rope_kv_write")
    sl = torch.tensor(slots, dtype=torch.long, device=dev)
    v = qkv[:, (H + KVH) * HD:].reshape(T, KVH, HD)
    assert torch.equal(p16.v[0][sl // PS, :, sl % PS], v.to(torch.bfloat16))   # V: exactly the rounded input
    # the switch off: an fp32 pool keeps the fp32 values (the default), a bf16 pool rounds whatever the switch says
    assert lib.fo_set_kv_bf16(0) in (0, 1)
    try:
        q32, q16 = _pools(dev)
        for pool in (q32, q16):
            ops.rope_kv_write(qkv, T, H, KVH, HD, pos, slot, cos, sin, qs[0], pool.k[0], pool.v[0], PS)
        torch.cuda.synchronize()
    finally:
        lib.fo_set_kv_bf16(prev)
    assert torch.equal(q32.v[0][sl // PS, :, sl % PS], v)
    assert torch.equal(q16.k, p16.k) and torch.equal(q16.v, p16.v)
