"""fo_gemm_w6_rows (the MXFP6 weight stream for 17..64 rows, PackedLinearW6(stream_rows=64)): tests/test_gemm_w4_rows_gpu.py's
cases on MXFP6, and the packed layout pinned exactly.  Every epilogue against float64 on the CPU definition's W'
(fo.quant.quantize_blocks_e2m3) with the tolerances of the bf16, FP8 and MXFP4 GEMM tests (rtol = atol = 1e-4: the
arithmetic is the same bf16 MFMAs on an exact decode), the same product as the bf16 image, K % 128 != 0 with nothing
read past K, rows beyond M, determinism, the host-side refusals and the default dispatch.  Every PackedLinearW6 here
sends all 17..64 rows to the row stream (stream = True, rows_rb = (2, 3, 4)), whatever the measured dispatch policy
keeps on the image; each test pins the entry's own counter, the <= 16-row MXFP6 counters and the bf16 kinds."""
import ctypes
import functools

import pytest
import torch

from test_gemm_w6_gpu import _weight

pytestmark = pytest.mark.gpu

BF16_KINDS = ("gemm_xsk", "gemm_rows")   # what the bf16 image runs at 17..64 rows


def _lin(dev, w, up=None):
    from fo.ops import PackedLinearW6
    p = PackedLinearW6(w.to(dev), swiglu_up=None if up is None else up.to(dev), stream_rows=64)
    p.stream = True
    p.rows_rb = (2, 3, 4)
    return p


def _counts():
    from fo import ops
    c = ops.launch_counts()
    return ops.w6_rows_launch_count(), ops.w6_launch_counts(), {k: c[k] for k in BF16_KINDS}


def _rose(before, n, free_bf16=False):
    """Since `before` = _counts(), the row stream's count rose by n; the <= 16-row MXFP6 forms and (unless free_bf16)
    the bf16 kinds did not move."""
    now = _counts()
    assert now[0] == before[0] + n, (before[0], now[0], n)
    assert now[1] == before[1]
    assert free_bf16 or now[2] == before[2]


def _swiglu(N, K, M, seed, gs=1, us=2, block_scaled=False):
    (wg, gdq), (wu, udq) = _weight(N, K, gs, block_scaled), _weight(N, K, us, block_scaled)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed))
    return wg, wu, x, torch.nn.functional.silu(x.double() @ gdq.t()) * (x.double() @ udq.t())


@functools.lru_cache(maxsize=None)
def _exact(M, N, K):
    """(bf16 weight, X, residual) on which every partial sum of X . W^T is exact in fp32 in any order: the weight is
    multiples of 0.5 in [-7.5, 7.5] times 2^-(block mod 3) per 32-column block, X integers in [-2, 2], the residual
    integers.  Every product is a multiple of 2^-3 and sum |x w| * 8 <= 120 K < 2^24."""
    g = torch.Generator().manual_seed(M + N + K)
    w = torch.randint(-15, 16, (N, K), generator=g).float() * 0.5
    w = (w * (2.0 ** -(torch.arange(K // 32) % 3).float()).repeat_interleave(32)[None]).to(torch.bfloat16)
    x = torch.randint(-2, 3, (M, K), generator=g).float()
    r = torch.randint(-9, 10, (M, N), generator=g).float()
    return w, x, r


@pytest.mark.parametrize("M,N,K", [(17, 48, 96), (33, 100, 160), (64, 176, 3584), (40, 272, 18944)])
def test_exact_layout(dev, M, N, K):
    """The code layout's k order, the block scales, the planes and the split-K slabs, bit for bit: on _exact's inputs
    the quantiser reproduces W, the float64 product is an fp32 number, and the plain and + Y outputs must equal it and
    the bf16 image's.  A wrong k assignment, block scale, plane or slab shows as a whole-number error here that a
    tolerance could hide."""
    from fo.quant import quantize_blocks_e2m3
    w, x, r = _exact(M, N, K)
    assert torch.equal(quantize_blocks_e2m3(w)[2].float(), w.float())          # W' == W
    ref = x.double() @ w.double().t()
    assert torch.equal(ref, ref.float().double()) and (x.abs().double() @ w.abs().double().t()).max() * 8 < 2 ** 24
    p = _lin(dev, w)
    xd = x.to(dev)
    before = _counts()
    y = p(xd)
    out = r.clone().to(dev)
    p(xd, out=out, residual=True)
    _rose(before, 2)
    bad = (y.cpu().double() != ref).nonzero()
    assert torch.equal(y.cpu().double(), ref), (bad[:8].tolist(), len(bad))
    assert torch.equal(out.cpu().double(), ref + r.double())
    assert torch.equal(y, p.bf16(xd))
    assert torch.equal(out, p.bf16(xd, out=r.clone().to(dev), residual=True))


def test_exact_layout_code_buffer_wraps(dev):
    """2256 columns at the down's K: 141 tiles, 71 pairs over the few workgroups a K slice gets, so every workgroup
    takes more than two units and the two-deep code buffer wraps; the last pair's second tile is out of range.
    Against the image only (the same exact inputs: any order of the partial sums gives the same bits), but for the
    last tile, the odd one, which float64 pins as well."""
    M, N, K = 40, 2256, 18944
    w, x, r = _exact(M, N, K)
    p = _lin(dev, w)
    xd = x.to(dev)
    before = _counts()
    y = p(xd)
    out = r.clone().to(dev)
    p(xd, out=out, residual=True)
    _rose(before, 2)
    assert torch.equal(y[:, -16:].cpu().double(), x.double() @ w[-16:].double().t())
    assert torch.equal(y, p.bf16(xd))
    assert torch.equal(out, p.bf16(xd, out=r.clone().to(dev), residual=True))


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


def _in_nan_buffer(x, dev):
    """x as a view of a wider device buffer whose columns at and beyond K hold NaN: they are never read."""
    M, K = x.shape
    xb = torch.full((M, K + 96), float("nan"))
    xb[:, :K] = x
    return xb.to(dev)[:, :K]


def test_swiglu_general_k(dev):
    """K % 128 == 32: three lane groups of the last code step hold blocks past K, which must meet no X."""
    M, N, K = 20, 200, 160
    wg, wu, x, ref = _swiglu(N, K, M, 9, 3, 4, True)
    before = _counts()
    y = _lin(dev, wg, wu)(_in_nan_buffer(x, dev))
    _rose(before, 1)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("M,N,K", [(17, 100, 96), (33, 3584, 256)])
def test_plain_general_k(dev, M, N, K):
    """(17, 100, 96): K % 128 == 96, lane group 3 of the only code step lies past K.  X in a NaN-padded buffer; at
    K = 96 also allocated exactly [M, K], contiguous, so that the last row ends where the buffer ends.  Block-scaled
    weights: another block's scale cannot pass."""
    w, wdq = _weight(N, K, 100 + N, True)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M + K))
    ref = x.double() @ wdq.t()
    p = _lin(dev, w)
    before = _counts()
    y = p(_in_nan_buffer(x, dev))
    _rose(before, 1)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    if K == 96:
        xe = x.to(dev)
        assert xe.is_contiguous() and xe.shape == (M, K)
        ye = p(xe)
        _rose(before, 2)
        assert torch.equal(ye, y)


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


@pytest.mark.parametrize("chain", ["w6_w6swiglu", "w6_bf16", "bf16_w6"])
@pytest.mark.parametrize("M", [24, 64])
def test_rmsnorm_across_gemms(dev, M, chain):
    """tests/test_gemm_w4_rows_gpu.py test_rmsnorm_across_gemms, its bounds, with the MXFP6 sides on the row stream
    (the bf16 sides run whatever fo_gemm picks for them, so only the MXFP6 counters are pinned)."""
    from fo import ops
    from fo.ops import PackedLinear
    D = 3584
    g = torch.Generator().manual_seed(M)
    (wp, pdq), (wc, cdq), (wu, udq) = _weight(D, 1024, 20), _weight(4096, D, 21), _weight(4096, D, 22)
    gamma = torch.rand(D, generator=g) + 0.5
    xin, res = torch.randn(M, 1024, generator=g), torch.randn(M, D, generator=g)
    p6, c6, sw = chain.startswith("w6"), chain != "w6_bf16", chain == "w6_w6swiglu"
    prod = _lin(dev, wp) if p6 else PackedLinear(wp.to(dev))
    cons = _lin(dev, wc, wu if sw else None) if c6 else PackedLinear(wc.to(dev))
    st = ops.RowStats(M, dev)
    x = res.clone().to(dev)
    yg = torch.empty(M, D, device=dev)
    before = _counts()
    prod(xin.to(dev), out=x, residual=True, stats_out=st.set(gamma.to(dev), yg))
    out = cons(yg, norm=(st, 1e-6))
    _rose(before, int(p6) + int(c6), free_bf16=True)
    y = res.double() + xin.double() @ (pdq if p6 else wp.double()).t()
    h = y * torch.rsqrt((y * y).mean(-1, keepdim=True) + 1e-6) * gamma.double()
    wcd = cdq if c6 else wc.double()
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
    _lib.call("fo_gemm_w6_rows", x.data_ptr(), x.stride(0), M, K, p.q.data_ptr(), p.scales.data_ptr(), p.ntiles, N, 0,
              out.data_ptr(), out.stride(0), 0, rt.ws.data_ptr(), ws_floats, rt.counters.data_ptr(), None, 0, 0.0, None,
              None, None, ctypes.byref(ctypes.c_int(0)), ops.stream(dev))


def test_refusals_are_host_side(dev):
    """A row count on either side of the band and a workspace of one float at the down's K: refused with the entry's
    text, nothing launched, nothing counted."""
    from fo import ops
    from fo.ops import PackedLinearW6
    w, _ = _weight(100, 96, 200)
    with pytest.raises(ValueError):
        PackedLinearW6(w.to(dev), stream_rows=32)
    with pytest.raises(ValueError):
        PackedLinearW6(w.to(dev), kind="head", stream_rows=64)      # a head stays at 16
    p = _lin(dev, w)
    x = torch.randn(80, 96, device=dev)
    out = torch.empty(80, 100, device=dev)
    long_k = _lin(dev, _weight(272, 18944, 100 + 272)[0])
    xl = torch.randn(40, 18944, device=dev)
    outl = torch.empty(40, 272, device=dev)
    rt = ops.Runtime.get(dev)
    before, before6 = ops.launch_counts(), _counts()
    for M in (16, 65):
        with pytest.raises(RuntimeError, match="17 <= M <= 64"):
            _raw(p, x, out, M, 96, 100, rt.ws.numel(), dev)
    with pytest.raises(RuntimeError, match="floats needed"):
        _raw(long_k, xl, outl, 40, 18944, 272, 1, dev)
    assert ops.launch_counts() == before
    assert _counts()[:2] == before6[:2]


def test_default_dispatch(dev):
    """A default PackedLinearW6 (stream_rows 16) runs the bf16 image at 17 rows, even with rows_rb forced; one built
    with stream_rows=64 runs the image above 64 rows and fo_gemm_w6 up to 16."""
    from fo import ops
    from fo.ops import PackedLinearW6
    w, wdq = _weight(100, 96, 200)
    p = PackedLinearW6(w.to(dev))
    assert p.stream_rows == 16 and p.rows_rb == () and not p.streams(17)
    p.rows_rb = (2, 3, 4)   # (even forced: the option is what opens the band)
    assert not p.streams(17)
    x = torch.randn(128, 96, generator=torch.Generator().manual_seed(4))
    xd = x.to(dev)
    before = _counts()
    y = p(xd[:17])
    _rose(before, 0, free_bf16=True)
    assert torch.equal(y, p.bf16(xd[:17]))
    torch.testing.assert_close(y.cpu().double(), x[:17].double() @ wdq.t(), rtol=1e-4, atol=1e-4)
    q = _lin(dev, w)
    assert q.stream_rows == 64 and q.streams(17) and q.streams(64) and not q.streams(65)
    for rows in (65, 128):
        assert torch.equal(q(xd[:rows]), q.bf16(xd[:rows]))
    _rose(before, 0, free_bf16=True)
    w6 = ops.w6_launch_counts()["w6"]
    for rows in (8, 16):
        torch.testing.assert_close(q(xd[:rows]).cpu().double(), x[:rows].double() @ wdq.t(), rtol=1e-4, atol=1e-4)
    assert ops.w6_launch_counts()["w6"] == w6 + 2 and _counts()[0] == before[0]
