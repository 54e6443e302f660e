"""fo_gemm_w8_rows and fo_gemm_w8_rows128 (the FP8 weight streams for 17..64 and 65..128 rows,
PackedLinearW8(stream_rows=64 / 128)): every epilogue against float64 on the DEQUANTISED weight with the tolerances of
tests/test_gemm_w8_gpu.py (the bf16 GEMM tests'), the same product as the bf16 image, rows beyond M, determinism and
the host-side refusals.  The tests are written once, over the band (`band_tests`): this module runs them for band 64,
tests/test_gemm_w8_rows128_gpu.py for band 128.  Every PackedLinearW8 here sends all rows of its band to the FP8
kernels (gemm_w8_ref.lin), whatever the measured dispatch policy keeps on the image."""
import ctypes

import pytest
import torch

from gemm_w8_ref import BANDS, BF16_KINDS, _swiglu_ref, _weight, assert_rose, counts, lin

pytestmark = pytest.mark.gpu

# per band: the row counts of the tests that take one from a list, or one each
GENERAL_M = {64: 20, 128: 70}
PLAIN = {64: [(17, 100, 96), (40, 272, 18944), (64, 272, 8192), (33, 3584, 256)],
         128: [(65, 100, 96), (100, 272, 18944), (128, 272, 8192), (97, 3584, 256)]}
PRODUCER_M = {64: [17, 40], 128: [65, 100]}
IMAGE_M = {64: 48, 128: 112}
CHAIN_M = {64: [24, 64], 128: [72, 128]}
BEYOND = {64: (32, 19), 128: (128, 70)}          # (rows of the buffers, M)
DOWN_M = {64: 40, 128: 100}
REFUSED = {64: (17, 64, "17 <= M <= 64", 80), 128: (65, 128, "65 <= M <= 128", 160)}   # (.., .., text, buffer rows)


def _raw(entry, p, x, out, M, K, N, ws_floats, dev):
    from fo import _lib, ops
    rt = ops.Runtime.get(dev)
    _lib.call(entry, x.data_ptr(), x.stride(0), M, K, p.q.data_ptr(), p.scales.data_ptr(), p.ntiles, N, 0,
              out.data_ptr(), out.stride(0), 0, rt.ws.data_ptr(), ws_floats, rt.counters.data_ptr(), None, 0, 0.0, None,
              None, None, ctypes.byref(ctypes.c_int(0)), ops.stream(dev))


def band_tests(band):
    """{name: test} of the tests of one band (64 or 128), for a test module's globals()."""

    @pytest.mark.parametrize("N", [176, 4120])
    @pytest.mark.parametrize("M", BANDS[band]["rows"])
    def test_swiglu_k3584(dev, M, N):
        """One row into a row block, full row blocks and the band's last; 176 columns are 11 units ((gate, up) pairs);
        4120 are 258: more than one per workgroup and a ragged last tile."""
        K = 3584
        x, ref = _swiglu_ref(N, K, M, M)
        p = lin(dev, band, _weight(N, K, 1)[0], _weight(N, K, 2)[0])
        before = counts()
        y = p(x.to(dev))
        assert_rose(before, band, 1)
        torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)

    def test_swiglu_general_k(dev):
        """K % 64 == 32: the last code step's second half is zero codes and must meet no X."""
        M, N, K = GENERAL_M[band], 200, 160
        (wg, gdq), (wu, udq) = _weight(N, K, 3), _weight(N, K, 4)
        x = torch.randn(M, K, generator=torch.Generator().manual_seed(9))
        # X sits in a wider buffer whose columns at and beyond K hold NaN: they are never read
        xb = torch.full((M, K + 32), float("nan"))
        xb[:, :K] = x
        before = counts()
        y = lin(dev, band, wg, wu)(xb.to(dev)[:, :K])
        assert_rose(before, band, 1)
        ref = torch.nn.functional.silu(x.double() @ gdq.t()) * (x.double() @ udq.t())
        torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)

    @pytest.mark.parametrize("M,N,K", PLAIN[band])
    def test_plain_and_residual(dev, M, N, K):
        """272 columns are 17 tiles (a last column group / tile group that is not full); 18944 is the down's K: 296
        code steps, which no slice size divides evenly; K = 96 has fewer code steps (2) than any K split of band 128."""
        w, wdq = _weight(N, K, 100 + N)
        g = torch.Generator().manual_seed(M + K)
        x, r = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
        p = lin(dev, band, w)
        before = counts()
        y = p(x.to(dev))
        out = r.clone().to(dev)
        p(x.to(dev), out=out, residual=True)
        assert_rose(before, band, 2)
        ref = x.double() @ wdq.t()
        torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(out.cpu().double(), ref + r.double(), rtol=1e-4, atol=1e-4)

    @pytest.mark.parametrize("M", PRODUCER_M[band])
    def test_producer_epilogue_long_k(dev, M):
        """Residual + yg + row sums at the down's K, merged by the second launch: against float64, three runs
        bit-equal, the tickets left zeroed."""
        from fo import ops
        N, K = 272, 18944
        w, wdq = _weight(N, K, 100 + N)
        g = torch.Generator().manual_seed(M)
        x, r, gamma = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g), torch.rand(N, generator=g) + 0.5
        p = lin(dev, band, w)
        st = ops.RowStats(M, dev)
        runs = []
        before = counts()
        for _ in range(3):
            out, yg = r.clone().to(dev), torch.zeros(M, N, device=dev)
            p(x.to(dev), out=out, residual=True, stats_out=st.set(gamma.to(dev), yg))
            runs.append((out.cpu(), yg.cpu(), st.buf[:M * st.groups].cpu()))
        assert_rose(before, band, 3)
        assert st.groups == 17
        assert not ops.Runtime.get(dev).counters[:64].any()
        for o in runs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(o, runs[0]))
        ref = x.double() @ wdq.t() + r.double()
        torch.testing.assert_close(runs[0][0].double(), ref, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(runs[0][1].double(), ref * gamma.double(), rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(runs[0][2].view(M, 17).sum(1).double(), (ref * ref).sum(1), rtol=1e-4, atol=1e-4)

    def test_same_product_as_the_image(dev):
        M = IMAGE_M[band]
        x, _ = _swiglu_ref(176, 3584, M, M)
        sw = lin(dev, band, _weight(176, 3584, 1)[0], _weight(176, 3584, 2)[0])
        pl = lin(dev, band, _weight(272, 8192, 100 + 272)[0])
        xp = torch.randn(M, 8192, generator=torch.Generator().manual_seed(2)).to(dev)
        before = counts()
        ys, yp = sw(x.to(dev)), pl(xp)
        assert_rose(before, band, 2)
        torch.testing.assert_close(ys, sw.bf16(x.to(dev)), rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(yp, pl.bf16(xp), rtol=1e-4, atol=1e-4)

    @pytest.mark.parametrize("chain", ["w8_w8swiglu", "w8_bf16", "bf16_w8"])
    @pytest.mark.parametrize("M", CHAIN_M[band])
    def test_rmsnorm_across_gemms(dev, M, chain):
        """tests/test_gemm_w8_gpu.py test_rmsnorm_across_gemms with the FP8 sides on the band's kernels (the bf16
        sides run whatever fo_gemm picks for them, so only the FP8 counters are pinned)."""
        from fo import ops
        from fo.ops import PackedLinear
        D = 3584
        g = torch.Generator().manual_seed(M)
        (wp, pdq), (wc, cdq), (wu, udq) = _weight(D, 1024, 20), _weight(4096, D, 21), _weight(4096, D, 22)
        gamma = torch.rand(D, generator=g) + 0.5
        xin, res = torch.randn(M, 1024, generator=g), torch.randn(M, D, generator=g)
        p8, c8, sw = chain.startswith("w8"), chain != "w8_bf16", chain == "w8_w8swiglu"
        prod = lin(dev, band, wp) if p8 else PackedLinear(wp.to(dev))
        cons = lin(dev, band, wc, wu if sw else None) if c8 else PackedLinear(wc.to(dev))
        st = ops.RowStats(M, dev)
        x = res.clone().to(dev)
        yg = torch.empty(M, D, device=dev)
        before = counts()
        prod(xin.to(dev), out=x, residual=True, stats_out=st.set(gamma.to(dev), yg))
        out = cons(yg, norm=(st, 1e-6))
        assert_rose(before, band, int(p8) + int(c8), free=BF16_KINDS)
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
        R, M = BEYOND[band]
        w, _ = _weight(100, 96, 200)
        p = lin(dev, band, w)
        x = torch.randn(R, 96, generator=torch.Generator().manual_seed(1)).to(dev)
        out = torch.full((R, 100), 7.0, device=dev)
        yg = torch.full((R, 100), 7.0, device=dev)
        st = ops.RowStats(R, dev)
        st.buf.fill_(-1.0)
        before = counts()
        p(x, out=out, M=M, stats_out=st.set(torch.ones(100, device=dev), yg))
        assert_rose(before, band, 1)
        assert st.groups == 7
        assert (out[M:] == 7).all() and (yg[M:] == 7).all() and (st.buf[M * 7:] == -1).all()
        assert torch.equal(out[:M], yg[:M])
        torch.testing.assert_close(st.buf[:M * 7].view(M, 7).sum(1), (out[:M] ** 2).sum(1), rtol=1e-5, atol=1e-5)

    def test_deterministic_down_shape(dev):
        g = torch.Generator().manual_seed(3)
        M, N, K = DOWN_M[band], 3584, 18944
        p = lin(dev, band, (torch.randn(N, K, generator=g) / 100).to(torch.bfloat16))
        x = torch.randn(M, K, generator=g).to(dev)
        before = counts()
        ys = [p(x).cpu() for _ in range(5)]
        assert_rose(before, band, 5)
        for y in ys[1:]:
            assert torch.equal(y, ys[0])

    def test_refusals_are_host_side(dev):
        """A row count on either side of the band, and for band 128 (whose every call needs the workspace) a
        workspace of one float: refused with the band's text, nothing launched."""
        from fo import ops
        from fo.ops import PackedLinearW8
        entry = BANDS[band]["entry"]
        lo, hi, text, R = REFUSED[band]
        w, _ = _weight(100, 96, 200)
        with pytest.raises(ValueError):
            PackedLinearW8(w.to(dev), stream_rows=32)
        p = lin(dev, band, w)
        x = torch.randn(R, 96, device=dev)
        out = torch.empty(R, 100, device=dev)
        rt = ops.Runtime.get(dev)
        if band == 128:
            long_k = lin(dev, band, _weight(272, 18944, 100 + 272)[0])
            xl = torch.randn(100, 18944, device=dev)
            outl = torch.empty(100, 272, device=dev)
        before = ops.launch_counts()
        for M in (lo - 1, hi + 1):
            with pytest.raises(RuntimeError, match=text):
                _raw(entry, p, x, out, M, 96, 100, rt.ws.numel(), dev)
        if band == 128:
            with pytest.raises(RuntimeError, match="floats needed"):
                _raw(entry, long_k, xl, outl, 100, 18944, 272, 1, dev)
        assert ops.launch_counts() == before

    return {k: v for k, v in locals().items() if k.startswith("test_")}


globals().update(band_tests(64))
