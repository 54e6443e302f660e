"""fo_gemm_w8_head / fo_gemm_w4_head (the Qwen2 output head's <= 16-row code streams: the plain form of the
X-stationary persistent kernels at K = 3584) against float64 X . W'^T, W' the CPU definition's dequantised weight
(fo.quant).  The streams decode the codes to the exact bf16 W' and run the bf16 kernels' arithmetic, so the tolerance is
the project's GEMM tolerance (rtol = atol = 1e-4), as in tests/test_gemm_w8_gpu.py / test_gemm_w4_gpu.py.

Shapes: N = 117 (8 tiles = 4 units, a ragged last tile of 5 columns, fewer units than CUs); N = 144 (9 tiles: the last
unit's second tile is out of the descriptors' range); N = 16 (2 (CUs + 37) - 1) - 3 (an odd tile count and a ragged
tile again, CUs + 37 units: some workgroups run two units and others one -- the loop, the prefetch of the next unit
and the uneven deal)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 3584
FMTS = ("fp8", "mxfp4")
SENTINEL = -123456.75


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _big_n():
    return 16 * (2 * (_cus() + 37) - 1) - 3


def _raw(N, fmt, seed):
    """A bf16 [N, K] weight on the CPU.  fp8: row n times 2^-(13 (n mod 5)), so that a neighbouring row's (or a
    missing) column scale is off by a large power of two; mxfp4: block j times 2^-(j mod 7), as
    tests/test_gemm_w4_gpu.py, so that another block's scale cannot pass.  Magnitudes only shrink, so the tolerance
    keeps its meaning; for fp8 it is also applied relative to each output column's own scale (see _check)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    if fmt == "fp8":
        w = w * (2.0 ** (-13.0 * (torch.arange(N) % 5)))[:, None]
    else:
        w = w * (2.0 ** -(torch.arange(K // 32) % 7).float()).repeat_interleave(32)[None]
    return w.to(torch.bfloat16)


def _col_scale(N, fmt):
    """The power of two (<= 1) _raw put on each output column (1 for mxfp4): the 1e-4 tolerance is applied to Y / scale
    as well as to Y, so that the scaled-down columns are held as tightly as the unit ones (the division is exact)."""
    if fmt == "fp8":
        return (2.0 ** (-13.0 * (torch.arange(N) % 5))).double()
    return torch.ones(N, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _small(N, fmt):
    """(bf16 weight, float64 W' of the CPU definition) for the small shapes, shared between the tests."""
    from fo.quant import quantize_blocks_e2m1, quantize_rows_e4m3
    w = _raw(N, fmt, 1000 + N)
    dq = (quantize_rows_e4m3 if fmt == "fp8" else quantize_blocks_e2m1)(w)[2]
    return w, dq.double()


_HEADS = {}


def _head(dev, N, fmt):
    """(head object streaming at <= 16 rows whatever ops.HEAD_POLICY says, float64 W').  The big shape's W' is the
    device's dequantised weight, which test_quantiser_matches_the_cpu_definition holds to the CPU definition bit for
    bit."""
    from fo import ops
    if (N, fmt) not in _HEADS:
        cls = ops.PackedLinearW8 if fmt == "fp8" else ops.PackedLinearW4
        if N == _big_n():
            w = _raw(N, fmt, 77).to(dev)
            wdq = (ops.quant_w8 if fmt == "fp8" else ops.quant_w4)(w)[2].cpu().double()
        else:
            w, wdq = _small(N, fmt)
        lin = cls(w.to(dev), kind="head")
        lin.stream = True
        _HEADS[(N, fmt)] = (lin, wdq)
    return _HEADS[(N, fmt)]


@functools.lru_cache(maxsize=None)
def _x(M, ldx):
    """fp32 rows with a non-trivial low half (not bf16-representable), in a buffer of row stride ldx."""
    g = torch.Generator().manual_seed(10 * M + ldx)
    x = torch.randn(M, ldx, generator=g)
    assert not torch.equal(x.to(torch.bfloat16).float(), x)
    return x


def _counts():
    from fo import ops
    return ops.head_launch_counts(), ops.launch_counts(), ops.w4_launch_counts()


def _code_counts():
    """The counters of every launch that streams codes (the bf16 image's launches move others)."""
    h, l, w = _counts()
    return h, {k: v for k, v in l.items() if k.startswith("gemm_w8")}, w


def _check(y, x, wdq, N, fmt):
    ref = x.double() @ wdq.t()
    s = _col_scale(N, fmt)
    torch.testing.assert_close(y.double(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(y.double() / s, ref / s, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("fmt", FMTS)
def test_quantiser_matches_the_cpu_definition(dev, fmt):
    """Codes, scales and image of an N = 117 head equal the CPU definition bit for bit."""
    from fo import ops
    from fo.quant import (pack_codes, pack_codes_w4, pack_scales, pack_scales_w4, quantize_blocks_e2m1,
                          quantize_rows_e4m3)
    w, wdq = _small(117, fmt)
    lin, _ = _head(dev, 117, fmt)
    if fmt == "fp8":
        q, e, dq = quantize_rows_e4m3(w)
        assert torch.equal(lin.q.cpu(), pack_codes(q)) and torch.equal(lin.scales.cpu(), pack_scales(e))
        assert lin.fp8_nbytes == 8 * 56 * 1024 + 8 * 16 * 4
    else:
        q, e, dq = quantize_blocks_e2m1(w)
        assert torch.equal(lin.q.cpu(), pack_codes_w4(q)) and torch.equal(lin.scales.cpu(), pack_scales_w4(e))
        assert lin.fp4_nbytes == 8 * 28 * 1024 + 8 * 28 * 64
    assert lin.ntiles == 8 and lin.kind == "head" and lin.stream_rows == 16 and lin.rows_rb == ()
    assert torch.equal(lin.packed, ops.PackedLinear(dq.to(dev)).packed)
    assert lin.nbytes == lin.bf16.nbytes


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M", [1, 7, 16])
@pytest.mark.parametrize("shape", ["117", "144", "big"])
def test_head_against_float64(dev, shape, M, fmt):
    """Every shape at every M; the output buffer has 16 rows of a sentinel: rows >= M and columns N..ldy keep it bit for
    bit.  ldx > K and ldy > N at M = 7.  One head launch per call, no other counter moves, two runs are equal."""
    N = _big_n() if shape == "big" else int(shape)
    lin, wdq = _head(dev, N, fmt)
    ldx, ldy = (K + 8, N + 5) if M == 7 else (K, N)
    xb = _x(M, ldx).to(dev)
    x = xb[:, :K]
    buf = torch.full((16, ldy), SENTINEL, device=dev)
    h0, l0, w0 = _counts()
    y = lin(x, out=buf[:, :N], M=M)
    h1, l1, w1 = _counts()
    slot = "w8_head" if fmt == "fp8" else "w4_head"
    assert h1 == {k: v + (k == slot) for k, v in h0.items()} and l1 == l0 and w1 == w0
    assert y.data_ptr() == buf.data_ptr()
    got = buf.cpu()
    assert (got[M:] == SENTINEL).all() and (got[:, N:] == SENTINEL).all()
    _check(got[:M, :N], x.cpu(), wdq, N, fmt)
    again = torch.full((16, ldy), SENTINEL, device=dev)
    lin(x, out=again[:, :N], M=M)
    assert torch.equal(again, buf)
    assert _counts()[0][slot] == h0[slot] + 2


@pytest.mark.parametrize("fmt", FMTS)
def test_17_rows_run_the_bf16_image(dev, fmt):
    from fo import ops
    lin, wdq = _head(dev, 144, fmt)
    x = _x(16, K + 8)[:, :K].contiguous()
    x = torch.cat([x, x[:1] * 0.5]).to(dev)
    before = _code_counts()
    y = lin(x)
    assert _code_counts() == before and not lin.streams(17) and lin.streams(16)
    assert torch.equal(y, ops.PackedLinear(wdq.to(torch.bfloat16).to(dev))(x))
    # 16 rows of the same weight stream the codes: the same product to the kernels' accumulation order
    y16 = lin(x[:16])
    assert sum(_code_counts()[0].values()) == sum(before[0].values()) + 1
    s = _col_scale(144, fmt).float().to(dev)
    torch.testing.assert_close(y16 / s, y[:16] / s, rtol=1e-4, atol=1e-4)
    # a format the policy keeps off the stream runs the image at every row count
    lin.stream = False
    try:
        mid = _code_counts()
        assert not lin.streams(8) and torch.equal(lin(x[:16]), lin.bf16(x[:16])) and _code_counts() == mid
    finally:
        lin.stream = True


@pytest.mark.parametrize("fmt", FMTS)
def test_head_policy_and_other_k(dev, fmt):
    """The constructor takes its dispatch from ops.HEAD_POLICY at K = 3584; a head of another K (the tiny config's 128)
    streams through the general plain form of fo_gemm_w8 / fo_gemm_w4 and never the head entry."""
    from fo import ops
    cls = ops.PackedLinearW8 if fmt == "fp8" else ops.PackedLinearW4
    w, _ = _small(117, fmt)
    assert cls(w.to(dev), kind="head").stream == ops.HEAD_POLICY[fmt]
    with pytest.raises(ValueError):
        cls(w.to(dev), kind="tail")
    with pytest.raises(ValueError):
        cls(w.to(dev), swiglu_up=w.to(dev), kind="head")
    with pytest.raises(ValueError):
        cls(w.to(dev), stream_rows=64, kind="head")
    from fo.quant import quantize_blocks_e2m1, quantize_rows_e4m3
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(100, 128, generator=g) / 128 ** 0.5).to(torch.bfloat16)
    wdq = (quantize_rows_e4m3 if fmt == "fp8" else quantize_blocks_e2m1)(w)[2].double()
    lin = cls(w.to(dev), kind="head")
    assert lin.stream and lin.streams(16) and not lin.streams(17)
    x = torch.randn(5, 128, generator=g)
    h0, l0, w0 = _counts()
    y = lin(x.to(dev))
    h1, l1, w1 = _counts()
    assert h1 == h0
    if fmt == "fp8":
        assert l1["gemm_w8"] == l0["gemm_w8"] + 1 and w1 == w0
    else:
        assert w1["w4"] == w0["w4"] + 1 and l1 == l0
    torch.testing.assert_close(y.cpu().double(), x.double() @ wdq.t(), rtol=1e-4, atol=1e-4)
