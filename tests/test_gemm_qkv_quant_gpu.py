"""fo_gemm_w8_qkv_rope / fo_gemm_w4_qkv_rope (the fused q|k|v projection's <= 16-row code streams: bias, RoPE and the
paged-KV append in the epilogue) through ops.PackedQKVQuant, against float64 on the CPU definition's dequantised weight
(fo.quant).  The streams decode the codes to the exact bf16 W' and run the bf16 kernels' arithmetic, so the tolerance is
the project's GEMM tolerance (rtol = atol = 1e-4, tests/test_gemm_w8_gpu.py); with the RMSNorm consumer 2e-4 of the
largest reference magnitude; against the bf16 image's own kernel on the same inputs 1e-4 / 1e-4, the accumulation-order
difference.

Shapes (H, KVH, hd, K, M): (2, 1, 32, 128, 1) one tile pair per head and one MXFP4 code step; (3, 1, 64, 96, 5)
K % 64 == 32 for FP8 and a partial MXFP4 step with padded scale bytes; (4, 2, 128, 3584, 8 / 16) four pairs per head,
GQA and the 16-wave form; once the real width (28, 4, 128, 3584, 8)."""
import functools
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

FMTS = ("fp8", "mxfp4")
PS, NP = 16, 12
SENT = -1536.0   # bf16-representable (1.5 x 2^10), far from every value written
EPS = 1e-6
SHAPES = {"hd32": (2, 1, 32, 128, 1), "hd64": (3, 1, 64, 96, 5), "wide8": (4, 2, 128, 3584, 8),
          "wide16": (4, 2, 128, 3584, 16), "real": (28, 4, 128, 3584, 8)}


def _raw(N, K, fmt, seed):
    """A bf16 [N, K] weight on the CPU.  fp8: row n times 2^-(n mod 3), so that a neighbouring row's (or a missing)
    column scale is off by a factor of two or more; mxfp4: block j times 2^-(j mod 7), so that another block's scale
    cannot pass.  Magnitudes only shrink, so the tolerance keeps its meaning."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    if fmt == "fp8":
        w = w * (2.0 ** -(torch.arange(N) % 3).float())[:, None]
    else:
        w = w * (2.0 ** -(torch.arange(K // 32) % 7).float()).repeat_interleave(32)[None]
    return w.to(torch.bfloat16)


_LINS = {}


def _lin(dev, H, KVH, hd, K, fmt):
    """(PackedQKVQuant forced to stream, its raw weight, float64 W', fp32 bias), shared between the tests.  The real
    width's W' is the device quantiser's dequantised weight, which ops.quant_w8 / quant_w4's own tests hold to the CPU
    definition; every other shape's is the CPU definition's."""
    from fo import ops
    from fo.quant import quantize_blocks_e2m1, quantize_rows_e4m3
    key = (H, KVH, hd, K, fmt)
    if key not in _LINS:
        N = (H + 2 * KVH) * hd
        w = _raw(N, K, fmt, 100 * H + hd + K)
        g = torch.Generator().manual_seed(N)
        bias = torch.randn(N, generator=g) * 0.5
        if H == 28:
            wdq = (ops.quant_w8 if fmt == "fp8" else ops.quant_w4)(w.to(dev))[2].cpu().double()
        else:
            wdq = (quantize_rows_e4m3 if fmt == "fp8" else quantize_blocks_e2m1)(w)[2].double()
        lins = {}
        for b in (True, False):
            lin = ops.PackedQKVQuant(w.to(dev), bias.to(dev) if b else None, hd, fmt)
            assert lin.stream == ops.ATTN_POLICY[fmt]["qkv"]
            lin.stream = True
            lins[b] = lin
        _LINS[key] = (lins, w, wdq, bias)
    return _LINS[key]


@functools.lru_cache(maxsize=None)
def _tables(hd):
    from fo import tables
    return tables.rope_tables(1e6, hd, 4096, round_fp16=True)


def _slots(M, seed):
    """M distinct token slots in a shuffled order over shuffled pages, with page 5's first and last slot."""
    r = random.Random(seed)
    must = [5 * PS, 5 * PS + PS - 1, 0, PS - 1]
    rest = [s for s in range(NP * PS) if s not in must]
    r.shuffle(rest)
    sl = (must + rest)[:M]
    r.shuffle(sl)
    return sl


def _inputs(dev, M, K, hd, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K + 8, generator=g)                    # fp32 rows with a low half, row stride K + 8
    assert not torch.equal(x.to(torch.bfloat16).float(), x)
    pos = torch.randint(0, 4096, (M,), generator=g, dtype=torch.int32)
    pos[0] = 4095
    slots = _slots(M, seed)
    cos, sin = _tables(hd)
    return (x.to(dev)[:, :K], pos.to(dev), torch.tensor(slots, dtype=torch.int32).to(dev), slots, cos.to(dev),
            sin.to(dev))


def _producer(dev, M, K, seed):
    """A real producer GEMM ([M, 64] x [K, 64]^T with stats_out) -> (xg = y * gamma: the consumer's X, the RowStats it
    filled, float64 rstd of y)."""
    from fo import ops
    g = torch.Generator().manual_seed(seed)
    wp = (torch.randn(K, 64, generator=g) / 8).to(torch.bfloat16).to(dev)
    xin = torch.randn(M, 64, generator=g).to(dev)
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).to(dev)
    st = ops.RowStats(16, dev)
    y, xg = torch.empty(M, K, device=dev), torch.empty(M, K, device=dev)
    ops.PackedLinear(wp)(xin, out=y, M=M, stats_out=st.set(gamma, xg))
    assert st.groups > 0
    rstd = ((y.double() ** 2).mean(1) + EPS).rsqrt().cpu()
    return xg, st, rstd


def _reference(x, wdq, bias, rstd, pos, hd, H, KVH):
    """float64 (q [M, H * hd], k [M, KVH, hd], v [M, KVH, hd]) with the fp32 tables."""
    cos, sin = _tables(hd)
    M, half = x.shape[0], hd // 2
    y = x.double().cpu() @ wdq.t()
    if rstd is not None:
        y = y * rstd[:, None]
    if bias is not None:
        y = y + bias.double()
    y = y.view(M, H + 2 * KVH, hd)
    c, s = cos[pos.cpu().long()].double()[:, None], sin[pos.cpu().long()].double()[:, None]
    x1, x2 = y[..., :half], y[..., half:]
    rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    return rot[:, :H].reshape(M, H * hd), rot[:, H:H + KVH], y[:, H + KVH:]


def _pool(dev, KVH, hd, dtype=torch.float32):
    from fo.kv import KVPool
    p = KVPool(1, KVH, hd, NP, PS, dev, dtype=dtype)
    p.k.fill_(SENT)
    p.v.fill_(SENT)
    return p


def _written(pool, slots):
    """(K rows [M, KVH, hd], V rows) at the slots, after checking that every other element keeps the sentinel."""
    sl = torch.tensor(slots, dtype=torch.long, device=pool.k.device)
    mask = torch.zeros(NP, PS, dtype=torch.bool, device=pool.k.device)
    mask[sl // PS, sl % PS] = True
    out = []
    for c in (pool.k[0], pool.v[0]):                                # [page][KVH][PS][hd]
        assert bool((c[~mask[:, None, :, None].expand_as(c)].float() == SENT).all())
        rows = c[sl // PS, :, sl % PS]
        assert not bool((rows.float() == SENT).any())
        out.append(rows)
    return out


def _counts():
    from fo import ops
    return ops.qkv_quant_launch_counts(), ops.launch_counts(), ops.w4_launch_counts()


def _call(lin, x, M, pos, slot, cos, sin, pool, H, KVH, norm=None):
    q = torch.full((M + 1, H * lin.rope_hd), SENT, device=x.device)
    lin.qkv_rope(x, M, pos, slot, cos, sin, q, pool.k[0], pool.v[0], H, KVH, PS, norm=norm)
    return q


def _close(got, ref, consumer, what):
    if consumer:
        torch.testing.assert_close(got.double().cpu(), ref, rtol=0, atol=2e-4 * float(ref.abs().max()), msg=what)
    else:
        torch.testing.assert_close(got.double().cpu(), ref, rtol=1e-4, atol=1e-4, msg=what)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", ["hd32", "hd64", "wide8"])
def test_packing_matches_the_cpu_definition(dev, shape, fmt):
    """Device-packed codes, scales and image equal fo.quant's quantiser + pack_*_rope bit for bit."""
    from fo import ops, quant
    H, KVH, hd, K, _ = SHAPES[shape]
    lins, w, wdq, bias = _lin(dev, H, KVH, hd, K, fmt)
    lin = lins[True]
    N = (H + 2 * KVH) * hd
    if fmt == "fp8":
        q, e, dq = quant.quantize_rows_e4m3(w)
        assert torch.equal(lin.q.cpu(), quant.pack_codes_rope(q, hd))
        assert torch.equal(lin.scales.cpu(), quant.pack_scales_rope(e, hd))
        assert lin.fp8_nbytes == N // 16 * ((K + 63) // 64) * 1024 + N * 4 and lin.fp4_nbytes == 0
    else:
        q, e, dq = quant.quantize_blocks_e2m1(w)
        assert torch.equal(lin.q.cpu(), quant.pack_codes_rope_w4(q, hd))
        assert torch.equal(lin.scales.cpu(), quant.pack_scales_rope_w4(e, hd))
        assert lin.fp4_nbytes == N // 16 * ((K + 127) // 128) * (1024 + 64) and lin.fp8_nbytes == 0
    assert not torch.equal(dq, w)
    want = ops.PackedLinear(dq.to(dev), bias.to(dev), rope_hd=hd)
    assert torch.equal(lin.packed, want.packed) and torch.equal(lin.bias, want.bias)
    assert lin.nbytes == want.nbytes and lin.ntiles == N // 16 and lins[False].bias is None
    assert torch.equal(lins[False].packed, want.packed) and torch.equal(lins[False].q, lin.q)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("consumer", [False, True], ids=["plain", "consumer"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_qkv_rope_against_float64(dev, shape, with_bias, consumer, fmt):
    H, KVH, hd, K, M = SHAPES[shape]
    lins, _, wdq, bias = _lin(dev, H, KVH, hd, K, fmt)
    lin = lins[with_bias]
    x, pos, slot, slots, cos, sin = _inputs(dev, M, K, hd, 7 * M + hd)
    norm = rstd = None
    if consumer:
        x, st, rstd = _producer(dev, M, K, K + M)
        norm = (st, EPS)
    pool = _pool(dev, KVH, hd)
    c0, l0, w0 = _counts()
    q = _call(lin, x, M, pos, slot, cos, sin, pool, H, KVH, norm)
    c1, l1, w1 = _counts()
    name = "w8_qkv_rope" if fmt == "fp8" else "w4_qkv_rope"
    assert c1 == {k: v + (k == name) for k, v in c0.items()} and l1 == l0 and w1 == w0
    rq, rk, rv = _reference(x, wdq, bias if with_bias else None, rstd, pos, hd, H, KVH)
    assert bool((q[M] == SENT).all())                               # the row past M is untouched
    k, v = _written(pool, slots)
    _close(q[:M], rq, consumer, "q_out")
    _close(k, rk, consumer, "K")
    _close(v, rv, consumer, "V")
    # the bf16 image's kernel on the same inputs: the accumulation-order difference
    pool_b = _pool(dev, KVH, hd)
    qb = _call(lin.bf16, x, M, pos, slot, cos, sin, pool_b, H, KVH, norm)
    assert _counts()[0] == c1
    kb, vb = _written(pool_b, slots)
    for a, b in ((q[:M], qb[:M]), (k, kb), (v, vb)):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)
    # determinism: the same call twice gives equal bits
    pool2 = _pool(dev, KVH, hd)
    q2 = _call(lin, x, M, pos, slot, cos, sin, pool2, H, KVH, norm)
    assert torch.equal(q2, q) and torch.equal(pool2.k, pool.k) and torch.equal(pool2.v, pool.v)
    assert _counts()[0][name] == c0[name] + 2


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", ["hd64", "wide16"])
def test_bf16_pool_holds_the_rounded_values(dev, shape, fmt):
    """kv_bytes = 2: the pool equals the bf16 rounding of what the same kernel wrote to an fp32 pool, and the fp32 pool
    under fo_set_kv_bf16(1) widened; q_out is equal in all three."""
    from fo import _lib
    H, KVH, hd, K, M = SHAPES[shape]
    lin = _lin(dev, H, KVH, hd, K, fmt)[0][True]
    x, pos, slot, slots, cos, sin = _inputs(dev, M, K, hd, 3 * M + hd)
    lib = _lib.load()
    prev = lib.fo_set_kv_bf16(0)
    try:
        p32, p16 = _pool(dev, KVH, hd), _pool(dev, KVH, hd, torch.bfloat16)
        q32 = _call(lin, x, M, pos, slot, cos, sin, p32, H, KVH)
        q16 = _call(lin, x, M, pos, slot, cos, sin, p16, H, KVH)
        assert lib.fo_set_kv_bf16(1) == 0
        pvb = _pool(dev, KVH, hd)
        qvb = _call(lin, x, M, pos, slot, cos, sin, pvb, H, KVH)
        torch.cuda.synchronize()
    finally:
        lib.fo_set_kv_bf16(prev)
    assert torch.equal(q32, q16) and torch.equal(q32, qvb)
    (k32, v32), (k16, v16), (kvb, vvb) = _written(p32, slots), _written(p16, slots), _written(pvb, slots)
    assert k16.dtype == torch.bfloat16 and not torch.equal(k32, k32.to(torch.bfloat16).float())
    assert torch.equal(k16, k32.to(torch.bfloat16)) and torch.equal(v16, v32.to(torch.bfloat16))
    assert torch.equal(kvb, k16.float()) and torch.equal(vvb, v16.float())
    assert torch.equal(p16.k.float(), pvb.k) and torch.equal(p16.v.float(), pvb.v)


@pytest.mark.parametrize("fmt", FMTS)
def test_17_rows_run_the_bf16_image(dev, fmt):
    from fo import ops
    H, KVH, hd, K, _ = SHAPES["wide16"]
    lins, _, wdq, bias = _lin(dev, H, KVH, hd, K, fmt)
    lin = lins[True]
    M = 17
    x, pos, slot, slots, cos, sin = _inputs(dev, M, K, hd, 17)
    ref = ops.PackedLinear(wdq.to(torch.bfloat16).to(dev), bias.to(dev), rope_hd=hd)
    assert not lin.streams(17) and lin.streams(16)
    before = _counts()[0]
    pa, pb = _pool(dev, KVH, hd), _pool(dev, KVH, hd)
    qa = _call(lin, x, M, pos, slot, cos, sin, pa, H, KVH)
    qb = _call(ref, x, M, pos, slot, cos, sin, pb, H, KVH)
    assert _counts()[0] == before
    assert torch.equal(qa, qb) and torch.equal(pa.k, pb.k) and torch.equal(pa.v, pb.v)
    # a bf16 input runs the image too, and so does every call of an instance the policy keeps off the stream
    pc, pd = _pool(dev, KVH, hd), _pool(dev, KVH, hd)
    xb = x[:8].to(torch.bfloat16)
    assert torch.equal(_call(lin, xb, 8, pos, slot, cos, sin, pc, H, KVH), _call(ref, xb, 8, pos, slot, cos, sin, pd, H, KVH))
    lin.stream = False
    try:
        assert not lin.streams(8)
        assert torch.equal(_call(lin, x, 8, pos, slot, cos, sin, pc, H, KVH), _call(ref, x, 8, pos, slot, cos, sin, pd, H, KVH))
    finally:
        lin.stream = True
    assert _counts()[0] == before and torch.equal(pc.k, pd.k)


@pytest.mark.parametrize("fmt", FMTS)
def test_attention_output_kind(dev, fmt):
    """kind="attn_o": plain, stream_rows 16, no row-stream policy, `.stream` from ops.ATTN_POLICY; forced to stream, a
    <= 16-row call with the residual and stats_out runs the general form of fo_gemm_w8 / fo_gemm_w4."""
    from fo import ops
    from fo.quant import quantize_blocks_e2m1, quantize_rows_e4m3
    cls = ops.PackedLinearW8 if fmt == "fp8" else ops.PackedLinearW4
    N = K = 3584
    w = _raw(N, K, fmt, 5)
    wdq = (quantize_rows_e4m3 if fmt == "fp8" else quantize_blocks_e2m1)(w)[2].double()
    lin = cls(w.to(dev), kind="attn_o")
    assert lin.kind == "attn_o" and lin.stream_rows == 16 and lin.rows_rb == ()
    assert lin.stream == ops.ATTN_POLICY[fmt]["o"] and not lin.streams(17)
    with pytest.raises(ValueError):
        cls(w.to(dev), swiglu_up=w.to(dev), kind="attn_o")
    with pytest.raises(ValueError):
        cls(w.to(dev), stream_rows=64, kind="attn_o")
    lin.stream = True
    g = torch.Generator().manual_seed(9)
    M = 8
    x = torch.randn(M, K, generator=g).to(dev)
    res = torch.randn(M, N, generator=g).to(dev)
    gamma = (1 + 0.1 * torch.randn(N, generator=g)).to(dev)
    out, yg, st = res.clone(), torch.empty(M, N, device=dev), ops.RowStats(16, dev)
    _, l0, w0 = _counts()
    lin(x, out=out, residual=True, M=M, stats_out=st.set(gamma, yg))
    _, l1, w1 = _counts()
    if fmt == "fp8":
        assert l1["gemm_w8"] == l0["gemm_w8"] + 1 and w1 == w0
    else:
        assert w1["w4"] == w0["w4"] + 1 and l1 == l0
    ref = x.double().cpu() @ wdq.t() + res.double().cpu()
    torch.testing.assert_close(out.double().cpu(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(yg.double().cpu(), ref * gamma.double().cpu(), rtol=1e-4, atol=1e-4)
    assert st.groups == N // 16
    sums = st.buf[:M * st.groups].view(M, st.groups).double().sum(1).cpu()      # [row][group] sums of squares
    torch.testing.assert_close(sums, (ref ** 2).sum(1), rtol=1e-4, atol=1e-4)
