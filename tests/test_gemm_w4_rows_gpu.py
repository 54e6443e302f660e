"""fo_gemm_w4_rows (the MXFP4 weight stream for 17..64 rows, PackedLinearW4(stream_rows=64)): tests/test_gemm_w8_rows_gpu.py's
band-64 cases on MXFP4.  Every epilogue against float64 on the CPU definition's W' (fo.quant.quantize_blocks_e2m1) with
the tolerances of the bf16 and FP8 GEMM tests (the arithmetic is the same bf16 MFMAs on an exact decode), the same
product as the bf16 image, rows beyond M, determinism, the host-side refusals and the default dispatch.  Every
PackedLinearW4 here sends all 17..64 rows to the row stream (rows_rb = (2, 3, 4)), whatever the measured dispatch
policy keeps on the image; each test pins the entry's own counter, the <= 16-row MXFP4 counters and the bf16 kinds."""
import ctypes

import pytest
import torch

from test_gemm_w4_gpu import _weight

pytestmark = pytest.mark.gpu

BF16_KINDS = ("gemm_xsk", "gemm_rows")   # what the bf16 image runs at 17..64 rows


def _lin(dev, w, up=None):
    from fo.ops import PackedLinearW4
    p = PackedLinearW4(w.to(dev), swiglu_up=None if up is None else up.to(dev), stream_rows=64)
    p.stream = True
    p.rows_rb = (2, 3, 4)
    return p


def _counts():
    from fo import ops
    c = ops.launch_counts()
    return ops.w4_rows_launch_count(), ops.w4_launch_counts(), {k: c[k] for k in BF16_KINDS}


def _rose(before, n, free_bf16=False):
    """Since `before` = _counts(), the row stream's count rose by n; the <= 16-row MXFP4 forms and (unless free_bf16)
    the bf16 kinds did not move."""
    now = _counts()
    assert now[0] == before[0] + n, (before[0], now[0], n)
    assert now[1] == before[1]
    assert free_bf16 or now[2] == before[2]


def _swiglu(N, K, M, seed, gs=1, us=2):
    (wg, gdq), (wu, udq) = _weight(N, K, gs), _weight(N, K, us)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed))
    return wg, wu, x, torch.nn.functional.silu(x.double() @ gdq.t()) * (x.double() @ udq.t())


@pytest.mark.parametrize("N", [176, 4120])
@pytest.mark.parametrize("M", [17, 32, 33, 48, 49, 64])
def test_swiglu_k3584(dev, M, N):
    """One row into a row block, full row blocks and the band's last; 176 columns are 11 units ((gate, up) pairs):
    fewer than the workgroups; 4120 are 258: more than one per workgroup and a ragged last tile."""
    wg, wu, x, ref = _swiglu(N, 3584, M, M)
    p = _lin(dev, wg, wu)
    before = _counts()
    y = p(x.to(dev))
    _rose(before, 1)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_swiglu_general_k(dev):
    """K % 128 == 32: three k-steps of the last code step are zero codes and must meet no X."""
    M, N, K = 20, 200, 160
    wg, wu, x, ref = _swiglu(N, K, M, 9, 3, 4)
    # X sits in a wider buffer whose columns at and beyond K hold NaN: they are never read
    xb = torch.full((M, K + 96), float("nan"))
    xb[:, :K] = x
    before = _counts()
    y = _lin(dev, wg, wu)(xb.to(dev)[:, :K])
    _rose(before, 1)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("block_scaled", [False, True])
@pytest.mark.parametrize("M,N,K", [(17, 100, 96), (40, 272, 18944), (64, 272, 8192), (33, 3584, 256)])
def test_plain_and_residual(dev, M, N, K, block_scaled):
    """(17, 100, 96): less than one code step, fewer steps than waves, a ragged N; (40, 272, 18944): the down's K, 148
    code steps that no slice size divides, and 17 tiles: the last pair's second tile is out of range; (33, 3584, 256):
    2 code steps, the in-kernel epilogue.  block_scaled: another block's scale cannot pass."""
    w, wdq = _weight(N, K, 100 + N, block_scaled)
    g = torch.Generator().manual_seed(M + K)
    x, r = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    p = _lin(dev, w)
    before = _counts()
    y = p(x.to(dev))
    out = r.clone().to(dev)
    p(x.to(dev), out=out, residual=True)
    _rose(before, 2)
    ref = x.double() @ wdq.t()
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.cpu().double(), ref + r.double(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("M", [17, 40])
def test_producer_epilogue_long_k(dev, M):
    """Residual + yg + row sums at the down's K, merged by the second launch: against float64, three runs bit-equal,
    the tickets left zeroed."""
    from fo import ops
    N, K = 272, 18944
    w, wdq = _weight(N, K, 100 + N)
    g = torch.Generator().manual_seed(M)
    x, r, gamma = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g), torch.rand(N, generator=g) + 0.5
    p = _lin(dev, w)
    st = ops.RowStats(M, dev)
    runs = []
    before = _counts()
    for _ in range(3):
        out, yg = r.clone().to(dev), torch.zeros(M, N, device=dev)
        p(x.to(dev), out=out, residual=True, stats_out=st.set(gamma.to(dev), yg))
        runs.append((out.cpu(), yg.cpu(), st.buf[:M * st.groups].cpu()))
    _rose(before, 3)
    assert st.groups == 17
    assert not ops.Runtime.get(dev).counters[:64].any()
    for o in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, runs[0]))
    ref = x.double() @ wdq.t() + r.double()
    torch.testing.assert_close(runs[0][0].double(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(runs[0][1].double(), ref * gamma.double(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(runs[0][2].view(M, 17).sum(1).double(), (ref * ref).sum(1), rtol=1e-4, atol=1e-4)


def test_same_product_as_the_image(dev):
    M = 48
    wg, wu, x, _ = _swiglu(176, 3584, M, M)
    sw = _lin(dev, wg, wu)
    pl = _lin(dev, _weight(272, 8192, 100 + 272)[0])
    xp = torch.randn(M, 8192, generator=torch.Generator().manual_seed(2)).to(dev)
    before = _counts()
    ys, yp = sw(x.to(dev)), pl(xp)
    _rose(before, 2)
    torch.testing.assert_close(ys, sw.bf16(x.to(dev)), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(yp, pl.bf16(xp), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("chain", ["w4_w4swiglu", "w4_bf16", "bf16_w4"])
@pytest.mark.parametrize("M", [24, 64])
def test_rmsnorm_across_gemms(dev, M, chain):
    """tests/test_gemm_w8_rows_gpu.py test_rmsnorm_across_gemms, its bounds, with the MXFP4 sides on the row stream
    (the bf16 sides run whatever fo_gemm picks for them, so only the MXFP4 counters are pinned)."""
    from fo import ops
    from fo.ops import PackedLinear
    D = 3584
    g = torch.Generator().manual_seed(M)
    (wp, pdq), (wc, cdq), (wu, udq) = _weight(D, 1024, 20), _weight(4096, D, 21), _weight(4096, D, 22)
    gamma = torch.rand(D, generator=g) + 0.5
    xin, res = torch.randn(M, 1024, generator=g), torch.randn(M, D, generator=g)
    p4, c4, sw = chain.startswith("w4"), chain != "w4_bf16", chain == "w4_w4swiglu"
    prod = _lin(dev, wp) if p4 else PackedLinear(wp.to(dev))
    cons = _lin(dev, wc, wu if sw else None) if c4 else PackedLinear(wc.to(dev))
    st = ops.RowStats(M, dev)
    x = res.clone().to(dev)
    yg = torch.empty(M, D, device=dev)
    before = _counts()
    prod(xin.to(dev), out=x, residual=True, stats_out=st.set(gamma.to(dev), yg))
    out = cons(yg, norm=(st, 1e-6))
    _rose(before, int(p4) + int(c4), free_bf16=True)
    y = res.double() + xin.double() @ (pdq if p4 else wp.double()).t()
    h = y * torch.rsqrt((y * y).mean(-1, keepdim=True) + 1e-6) * gamma.double()
    wcd = cdq if c4 else wc.double()
    ref = torch.nn.functional.silu(h @ wcd.t()) * (h @ udq.t()) if sw else h @ wcd.t()
    torch.testing.assert_close(x.cpu().double(), y, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(yg.cpu().double(), y * gamma.double(), rtol=1e-5, atol=1e-4)
    err = (out.cpu().double() - ref).abs().max().item()
    assert err < 2e-4 * ref.abs().max().item(), err


def test_rows_beyond_m_are_not_written(dev):
    """Rows >= M are computed from a clamped row: never stored, never added into the row sums."""
    from fo import ops
    R, M = 32, 19
    w, _ = _weight(100, 96, 200)
    p = _lin(dev, w)
    x = torch.randn(R, 96, generator=torch.Generator().manual_seed(1)).to(dev)
    out = torch.full((R, 100), 7.0, device=dev)
    yg = torch.full((R, 100), 7.0, device=dev)
    st = ops.RowStats(R, dev)
    st.buf.fill_(-1.0)
    before = _counts()
    p(x, out=out, M=M, stats_out=st.set(torch.ones(100, device=dev), yg))
    _rose(before, 1)
    assert st.groups == 7
    assert (out[M:] == 7).all() and (yg[M:] == 7).all() and (st.buf[M * 7:] == -1).all()
    assert torch.equal(out[:M], yg[:M])
    torch.testing.assert_close(st.buf[:M * 7].view(M, 7).sum(1), (out[:M] ** 2).sum(1), rtol=1e-5, atol=1e-5)


def test_deterministic_down_shape(dev):
    g = torch.Generator().manual_seed(3)
    M, N, K = 40, 3584, 18944
    p = _lin(dev, (torch.randn(N, K, generator=g) / 100).to(torch.bfloat16))
    x = torch.randn(M, K, generator=g).to(dev)
    before = _counts()
    ys = [p(x).cpu() for _ in range(5)]
    _rose(before, 5)
    for y in ys[1:]:
        assert torch.equal(y, ys[0])


def _raw(p, x, out, M, K, N, ws_floats, dev):
    from fo import _lib, ops
    rt = ops.Runtime.get(dev)
    _lib.call("fo_gemm_w4_rows", x.data_ptr(), x.stride(0), M, K, p.q.data_ptr(), p.scales.data_ptr(), p.ntiles, N, 0,
              out.data_ptr(), out.stride(0), 0, rt.ws.data_ptr(), ws_floats, rt.counters.data_ptr(), None, 0, 0.0, None,
              None, None, ctypes.byref(ctypes.c_int(0)), ops.stream(dev))


def test_refusals_are_host_side(dev):
    """A row count on either side of the band and a workspace of one float at the down's K: refused with the entry's
    text, nothing launched, nothing counted."""
    from fo import ops
    from fo.ops import PackedLinearW4
    w, _ = _weight(100, 96, 200)
    with pytest.raises(ValueError):
        PackedLinearW4(w.to(dev), stream_rows=32)
    p = _lin(dev, w)
    x = torch.randn(80, 96, device=dev)
    out = torch.empty(80, 100, device=dev)
    long_k = _lin(dev, _weight(272, 18944, 100 + 272)[0])
    xl = torch.randn(40, 18944, device=dev)
    outl = torch.empty(40, 272, device=dev)
    rt = ops.Runtime.get(dev)
    before, before4 = ops.launch_counts(), _counts()
    for M in (16, 65):
        with pytest.raises(RuntimeError, match="17 <= M <= 64"):
            _raw(p, x, out, M, 96, 100, rt.ws.numel(), dev)
    with pytest.raises(RuntimeError, match="floats needed"):
        _raw(long_k, xl, outl, 40, 18944, 272, 1, dev)
    assert ops.launch_counts() == before
    assert _counts()[:2] == before4[:2]


def test_default_dispatch_keeps_17_rows_on_the_image(dev):
    """A default PackedLinearW4 (stream_rows 16) runs the bf16 image at 17 rows."""
    from fo.ops import PackedLinearW4
    w, wdq = _weight(100, 96, 200)
    p = PackedLinearW4(w.to(dev))
    assert p.stream_rows == 16 and not p.streams(17)
    p.rows_rb = (2, 3, 4)   # (even forced: the option is what opens the band)
    assert not p.streams(17)
    x = torch.randn(17, 96, generator=torch.Generator().manual_seed(4))
    before = _counts()
    y = p(x.to(dev))
    _rose(before, 0, free_bf16=True)
    torch.testing.assert_close(y.cpu().double(), x.double() @ wdq.t(), rtol=1e-4, atol=1e-4)
