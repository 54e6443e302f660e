"""fo_gemm_w8_rows128 (the FP8 weight stream for 65..128 rows, PackedLinearW8(stream_rows=128)): every epilogue against
float64 on the DEQUANTISED weight with the tolerances of tests/test_gemm_w8_rows_gpu.py (the bf16 GEMM tests'), the
same product as the bf16 image, rows beyond M, determinism and the host-side refusals.  Every PackedLinearW8 here sends
all of 17..128 rows to the FP8 kernels (rows_rb), whatever the measured dispatch policy keeps on the image."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _weight(N, K, seed):
    """(bf16 weight, its dequantised FP8 image as float64), on the CPU, shared between the tests."""
    from fo.quant import quantize_rows_e4m3
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    return w, quantize_rows_e4m3(w)[2].double()


def _lin(dev, w, up=None):
    from fo.ops import PackedLinearW8
    lin = PackedLinearW8(w.to(dev), swiglu_up=None if up is None else up.to(dev), stream_rows=128)
    lin.rows_rb = tuple(range(2, 9))
    return lin


KINDS = ("gemm_w8_rows128", "gemm_w8_rows", "gemm_w8", "gemm_rows", "gemm_xsk")


def _counts():
    from fo import ops
    c = ops.launch_counts()
    return tuple(c[k] for k in KINDS)


def _rose(before, n):
    return _counts() == (before[0] + n,) + before[1:]


@functools.lru_cache(maxsize=None)
def _swiglu_ref(N, K, M, seed):
    (_, gdq), (_, udq) = _weight(N, K, 1), _weight(N, K, 2)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed))
    return x, torch.nn.functional.silu(x.double() @ gdq.t()) * (x.double() @ udq.t())


@pytest.mark.parametrize("N", [176, 4120])
@pytest.mark.parametrize("M", [65, 80, 81, 112, 113, 128])
def test_swiglu_k3584(dev, M, N):
    """One row into a row block, full row blocks and all 8; 176 columns are 11 (gate, up) pairs, 4120 are 258: several
    per workgroup and a ragged last tile."""
    K = 3584
    x, ref = _swiglu_ref(N, K, M, M)
    lin = _lin(dev, _weight(N, K, 1)[0], _weight(N, K, 2)[0])
    before = _counts()
    y = lin(x.to(dev))
    assert _rose(before, 1)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_swiglu_general_k(dev):
    """K % 64 == 32: the last code step's second half is zero codes and must meet no X."""
    M, N, K = 70, 200, 160
    (wg, gdq), (wu, udq) = _weight(N, K, 3), _weight(N, K, 4)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(9))
    # X sits in a wider buffer whose columns at and beyond K hold NaN: they are never read
    xb = torch.full((M, K + 32), float("nan"))
    xb[:, :K] = x
    before = _counts()
    y = _lin(dev, wg, wu)(xb.to(dev)[:, :K])
    assert _rose(before, 1)
    ref = torch.nn.functional.silu(x.double() @ gdq.t()) * (x.double() @ udq.t())
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("M,N,K", [(65, 100, 96), (100, 272, 18944), (128, 272, 8192), (97, 3584, 256)])
def test_plain_and_residual(dev, M, N, K):
    """272 columns are 17 tiles (a ragged last tile group); 18944 is the down's K: 296 code steps, uneven slices; K = 96
    has fewer code steps (2) than any K split."""
    w, wdq = _weight(N, K, 100 + N)
    g = torch.Generator().manual_seed(M + K)
    x, r = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    lin = _lin(dev, w)
    before = _counts()
    y = lin(x.to(dev))
    out = r.clone().to(dev)
    lin(x.to(dev), out=out, residual=True)
    assert _rose(before, 2)
    ref = x.double() @ wdq.t()
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.cpu().double(), ref + r.double(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("M", [65, 100])
def test_producer_epilogue_long_k(dev, M):
    """Residual + yg + row sums at the down's K: against float64, three runs bit-equal, the tickets left zeroed."""
    from fo import ops
    N, K = 272, 18944
    w, wdq = _weight(N, K, 100 + N)
    g = torch.Generator().manual_seed(M)
    x, r, gamma = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g), torch.rand(N, generator=g) + 0.5
    lin = _lin(dev, w)
    st = ops.RowStats(M, dev)
    runs = []
    before = _counts()
    for _ in range(3):
        out, yg = r.clone().to(dev), torch.zeros(M, N, device=dev)
        lin(x.to(dev), out=out, residual=True, stats_out=st.set(gamma.to(dev), yg))
        runs.append((out.cpu(), yg.cpu(), st.buf[:M * st.groups].cpu()))
    assert _rose(before, 3)
    assert st.groups == 17
    assert not ops.Runtime.get(dev).counters[:64].any()
    for o in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, runs[0]))
    ref = x.double() @ wdq.t() + r.double()
    torch.testing.assert_close(runs[0][0].double(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(runs[0][1].double(), ref * gamma.double(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(runs[0][2].view(M, 17).sum(1).double(), (ref * ref).sum(1), rtol=1e-4, atol=1e-4)


def test_same_product_as_the_image(dev):
    M = 112
    x, _ = _swiglu_ref(176, 3584, M, M)
    sw = _lin(dev, _weight(176, 3584, 1)[0], _weight(176, 3584, 2)[0])
    pl = _lin(dev, _weight(272, 8192, 100 + 272)[0])
    xp = torch.randn(M, 8192, generator=torch.Generator().manual_seed(2)).to(dev)
    before = _counts()
    ys, yp = sw(x.to(dev)), pl(xp)
    assert _rose(before, 2)
    torch.testing.assert_close(ys, sw.bf16(x.to(dev)), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(yp, pl.bf16(xp), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("chain", ["w8_w8swiglu", "w8_bf16", "bf16_w8"])
@pytest.mark.parametrize("M", [72, 128])
def test_rmsnorm_across_gemms(dev, M, chain):
    """tests/test_gemm_w8_rows_gpu.py test_rmsnorm_across_gemms with the FP8 sides on the 65..128-row kernel (the bf16
    sides run whatever fo_gemm picks for them, so only the FP8 counters are pinned)."""
    from fo import ops
    from fo.ops import PackedLinear
    D = 3584
    g = torch.Generator().manual_seed(M)
    (wp, pdq), (wc, cdq), (wu, udq) = _weight(D, 1024, 20), _weight(4096, D, 21), _weight(4096, D, 22)
    gamma = torch.rand(D, generator=g) + 0.5
    xin, res = torch.randn(M, 1024, generator=g), torch.randn(M, D, generator=g)
    p8, c8, sw = chain.startswith("w8"), chain != "w8_bf16", chain == "w8_w8swiglu"
    prod = _lin(dev, wp) if p8 else PackedLinear(wp.to(dev))
    cons = _lin(dev, wc, wu if sw else None) if c8 else PackedLinear(wc.to(dev))
    st = ops.RowStats(M, dev)
    x = res.clone().to(dev)
    yg = torch.empty(M, D, device=dev)
    before = _counts()
    prod(xin.to(dev), out=x, residual=True, stats_out=st.set(gamma.to(dev), yg))
    out = cons(yg, norm=(st, 1e-6))
    after = _counts()
    assert after[0] - before[0] == int(p8) + int(c8) and after[1:3] == before[1:3]
    y = res.double() + xin.double() @ (pdq if p8 else wp.double()).t()
    h = y * torch.rsqrt((y * y).mean(-1, keepdim=True) + 1e-6) * gamma.double()
    wcd = cdq if c8 else wc.double()
    ref = torch.nn.functional.silu(h @ wcd.t()) * (h @ udq.t()) if sw else h @ wcd.t()
    torch.testing.assert_close(x.cpu().double(), y, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(yg.cpu().double(), y * gamma.double(), rtol=1e-5, atol=1e-4)
    err = (out.cpu().double() - ref).abs().max().item()
    assert err < 2e-4 * ref.abs().max().item(), err


def test_rows_beyond_m_are_not_written(dev):
    """Rows >= M are computed from a clamped row: never stored, never added into the row sums."""
    from fo import ops
    w, _ = _weight(100, 96, 200)
    lin = _lin(dev, w)
    x = torch.randn(128, 96, generator=torch.Generator().manual_seed(1)).to(dev)
    out = torch.full((128, 100), 7.0, device=dev)
    yg = torch.full((128, 100), 7.0, device=dev)
    st = ops.RowStats(128, dev)
    st.buf.fill_(-1.0)
    before = _counts()
    lin(x, out=out, M=70, stats_out=st.set(torch.ones(100, device=dev), yg))
    assert _rose(before, 1)
    assert st.groups == 7
    assert (out[70:] == 7).all() and (yg[70:] == 7).all() and (st.buf[70 * 7:] == -1).all()
    assert torch.equal(out[:70], yg[:70])
    torch.testing.assert_close(st.buf[:70 * 7].view(70, 7).sum(1), (out[:70] ** 2).sum(1), rtol=1e-5, atol=1e-5)


def test_deterministic_down_shape(dev):
    g = torch.Generator().manual_seed(3)
    M, N, K = 100, 3584, 18944
    lin = _lin(dev, (torch.randn(N, K, generator=g) / 100).to(torch.bfloat16))
    x = torch.randn(M, K, generator=g).to(dev)
    before = _counts()
    ys = [lin(x).cpu() for _ in range(5)]
    assert _rose(before, 5)
    for y in ys[1:]:
        assert torch.equal(y, ys[0])


def _raw(lin, x, out, M, K, N, ws_floats, dev):
    from fo import _lib, ops
    rt = ops.Runtime.get(dev)
    _lib.call("fo_gemm_w8_rows128", x.data_ptr(), x.stride(0), M, K, lin.q.data_ptr(), lin.scales.data_ptr(),
              lin.ntiles, N, 0, out.data_ptr(), out.stride(0), 0, rt.ws.data_ptr(), ws_floats,
              rt.counters.data_ptr(), None, 0, 0.0, None, None, None, ctypes.byref(ctypes.c_int(0)), ops.stream(dev))


def test_refusals_are_host_side(dev):
    from fo import ops
    from fo.ops import PackedLinearW8
    w, _ = _weight(100, 96, 200)
    with pytest.raises(ValueError):
        PackedLinearW8(w.to(dev), stream_rows=32)
    lin = _lin(dev, w)
    x = torch.randn(160, 96, device=dev)
    out = torch.empty(160, 100, device=dev)
    rt = ops.Runtime.get(dev)
    long_k = _lin(dev, _weight(272, 18944, 100 + 272)[0])
    xl = torch.randn(100, 18944, device=dev)
    outl = torch.empty(100, 272, device=dev)
    before = ops.launch_counts()
    for M in (64, 129):
        with pytest.raises(RuntimeError, match="65 <= M <= 128"):
            _raw(lin, x, out, M, 96, 100, rt.ws.numel(), dev)
    with pytest.raises(RuntimeError, match="floats needed"):
        _raw(long_k, xl, outl, 100, 18944, 272, 1, dev)
    assert ops.launch_counts() == before
