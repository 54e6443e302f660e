"""fo_quant_w6 / fo_gemm_w6 / fo_gemm_w6_head (weight-only MXFP6 for <= 16 rows): the hardware decode and the packed
layout pinned exactly through one-hot products, the device quantiser against the CPU definition bit for bit, and every
form and epilogue of the GEMM against float64 X . W'^T on the CPU definition's W' -- the MXFP6 stream decodes the codes
to the exact bf16 W' and runs the bf16 kernels' arithmetic, so the tolerances are those of tests/test_gemm_w4_gpu.py
(rtol = atol = 1e-4)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _weight(N, K, seed, block_scaled=False):
    """(bf16 weight, its dequantised MXFP6 image as float64), on the CPU, shared between the tests.  block_scaled:
    block j of every row times 2^-(j mod 7), so that a kernel applying another block's scale is far off (magnitudes
    only shrink: the tolerance keeps its meaning)."""
    from fo.quant import quantize_blocks_e2m3
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    if block_scaled:
        w = w * (2.0 ** -(torch.arange(K // 32) % 7).float()).repeat_interleave(32)[None]
    w = w.to(torch.bfloat16)
    return w, quantize_blocks_e2m3(w)[2].double()


@functools.lru_cache(maxsize=None)
def _swiglu_ref(N, K, M):
    (_, gdq), (_, udq) = _weight(N, K, 1), _weight(N, K, 2)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M))
    return x, torch.nn.functional.silu(x.double() @ gdq.t()) * (x.double() @ udq.t())


def _lin(dev, w, up=None, kind=None):
    """PackedLinearW6 that streams the codes at <= 16 rows whatever the measured dispatch policy keeps on the image."""
    from fo.ops import PackedLinearW6
    p = PackedLinearW6(w.to(dev), swiglu_up=None if up is None else up.to(dev), kind=kind)
    p.stream = True
    return p


def _counts():
    from fo import ops
    c = ops.w6_launch_counts()
    return c["w6"], c["w6_xs"], c["w6_sk"], c["w6_head"]


def _others():
    from fo import ops
    return ops.launch_counts(), ops.w4_launch_counts(), ops.head_launch_counts()


def _rose(before, w6=0, xs=0, sk=0, head=0):
    assert _counts() == (before[0] + w6, before[1] + xs, before[2] + sk, before[3] + head)


def test_exact_decode_and_layout(dev):
    """A 64 x 128 weight whose 256 blocks together hold all 64 codes at all 32 positions, block j of a row under
    2^-(j mod 7) and row n under 2^(n mod 5 - 2): several scale bytes.  Every value is a grid point times its block's
    power of two and every block holds a magnitude >= 4, so the weight is its own image.  Multiplied by one-hot rows
    (8 launches of 16 rows; 1.0 splits into hi = 1, lo = 0 and every other product is 0 * finite), the outputs are W'
    itself: any mix-up of the convert's bit order, of the lanes' columns or of the scale bytes shows as an unequal
    element."""
    from fo.quant import E2M3_GRID, quantize_blocks_e2m3
    n, j, p = torch.meshgrid(torch.arange(64), torch.arange(4), torch.arange(32), indexing="ij")
    code = (p + 4 * n + j) % 64
    grid = torch.tensor(E2M3_GRID)
    val = torch.where(code >= 32, -grid[code % 32], grid[code % 32])
    w = torch.ldexp(val, -(j % 7) + n % 5 - 2).reshape(64, 128).to(torch.bfloat16)
    q, e, w_dq = quantize_blocks_e2m3(w)
    assert torch.equal(q.view(64, 4, 32).long(), code)                      # the construction: codes as intended
    assert torch.equal(e, (-(j % 7) + n % 5 - 2)[..., 0].int()) and e.unique().numel() >= 5
    for pos in range(32):
        assert code[..., pos].unique().numel() == 64
    assert torch.equal(w_dq.float(), w.float())
    lin = _lin(dev, w)
    eye = torch.eye(128, device=dev)
    before = _counts()
    cols = [lin(eye[16 * i:16 * i + 16].contiguous()) for i in range(8)]    # [16, 64] each: W'[:, 16 i .. + 16]^T
    _rose(before, w6=8)
    got = torch.cat(cols).t().cpu()
    bad = (got != w_dq.float()).nonzero()
    assert torch.equal(got, w_dq.float()), (bad[:8].tolist(), got[tuple(bad[0])] if len(bad) else None)


def test_quantiser_matches_the_cpu_definition(dev):
    from fo import ops
    from fo.quant import pack_codes_w6, pack_scales_w6, quantize_blocks_e2m3
    from test_quant_w6_cpu import edge_weight_w6
    g = torch.Generator().manual_seed(5)
    big = torch.randn(3584, 256, generator=g) * torch.exp(torch.randn(3584, 8, generator=g) * 3).repeat_interleave(32, 1)
    for w in (edge_weight_w6(), big.to(torch.bfloat16), big[:100, :96].contiguous()):   # (the last one fp32)
        q, e, w_dq = quantize_blocks_e2m3(w)
        for base, stride in ((0, 1), (1, 2)):
            qd, sd, dq = ops.quant_w6(w.to(dev), base, stride)
            assert torch.equal(qd.cpu(), pack_codes_w6(q, base, stride)), (tuple(w.shape), base)
            assert torch.equal(sd.cpu(), pack_scales_w6(e, base, stride)), (tuple(w.shape), base)
            assert dq.dtype == torch.bfloat16 and torch.equal(dq.cpu().view(torch.int16), w_dq.view(torch.int16))
    # the SwiGLU pair: gate and up tiles interleaved
    from fo.ops import PackedLinearW6
    wg, wu = edge_weight_w6(), edge_weight_w6().flip(0).contiguous()
    lin = PackedLinearW6(wg.to(dev), swiglu_up=wu.to(dev))
    (qg, eg, _), (qu, eu, _) = quantize_blocks_e2m3(wg), quantize_blocks_e2m3(wu)
    assert torch.equal(lin.q.cpu(), pack_codes_w6(qu, 1, 2, pack_codes_w6(qg, 0, 2, torch.zeros(lin.q.numel(), dtype=torch.uint8))))
    assert torch.equal(lin.scales.cpu(),
                       pack_scales_w6(eu, 1, 2, pack_scales_w6(eg, 0, 2, torch.zeros(lin.scales.numel(), dtype=torch.uint8))))
    assert lin.fp6_nbytes == lin.q.numel() + lin.scales.numel() == 4 * 1536 + 4 * 64 and lin.nbytes == lin.bf16.nbytes
    assert lin.stream_rows == 16 and lin.rows_rb == () and lin.kind is None


@pytest.mark.parametrize("block_scaled", [False, True])
@pytest.mark.parametrize("M,N,K", [(1, 64, 128), (3, 100, 96), (16, 48, 18944), (8, 3584, 256)])
def test_plain_and_residual(dev, M, N, K, block_scaled):
    """(3, 100, 96): a ragged N and K % 128 == 96, where lane group 3 of the only code step lies past K and the X
    buffer ends at the last row's column K; (16, 48, 18944): the down projection's K."""
    w, wdq = _weight(N, K, 100 + N, block_scaled)
    g = torch.Generator().manual_seed(M + K)
    x, r = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    lin = _lin(dev, w)
    before, others = _counts(), _others()
    y = lin(x.to(dev))
    out = r.clone().to(dev)
    lin(x.to(dev), out=out, residual=True)
    _rose(before, w6=2)
    assert _others() == others
    ref = x.double() @ wdq.t()
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.cpu().double(), ref + r.double(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("K", [32, 160, 192])
def test_blocks_past_k_read_no_x(dev, K):
    """K % 128 = 32, 32 and 64: the lanes of the last code step whose block lies at or past K must feed zeros, not what
    follows X[row, K:] -- here NaN in every row but the last (ldx > K), which would turn NaN * 0 into NaN."""
    M, N = 4, 40
    w, wdq = _weight(N, K, 400 + K)
    xb = torch.full((M, K + 128), float("nan"))
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(K))
    xb[:, :K] = x
    lin = _lin(dev, w)
    y = lin(xb.to(dev)[:, :K])
    torch.testing.assert_close(y.cpu().double(), x.double() @ wdq.t(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("N", [176, 4120])
@pytest.mark.parametrize("M", [1, 8, 16])
def test_swiglu_k3584(dev, M, N):
    """The X-stationary form; 4120 columns are 258 units: more than one per workgroup and a ragged last tile."""
    K = 3584
    x, ref = _swiglu_ref(N, K, M)
    lin = _lin(dev, _weight(N, K, 1)[0], _weight(N, K, 2)[0])
    before = _counts()
    y = lin(x.to(dev))
    _rose(before, xs=1)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_swiglu_general_form(dev):
    """The SwiGLU pair at another K runs the general form."""
    M, N, K = 5, 40, 256
    x, ref = _swiglu_ref(N, K, M)
    lin = _lin(dev, _weight(N, K, 1)[0], _weight(N, K, 2)[0])
    before = _counts()
    y = lin(x.to(dev))
    _rose(before, w6=1)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_swiglu_general_form_16_waves(dev):
    """17 code steps (K % 128 == 96): the SwiGLU pair on the general form's 16 waves."""
    M, N, K = 5, 40, 2144
    x, ref = _swiglu_ref(N, K, M)
    lin = _lin(dev, _weight(N, K, 1)[0], _weight(N, K, 2)[0])
    before = _counts()
    y = lin(x.to(dev))
    _rose(before, w6=1)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_swiglu_k3584_other_wave_shape():
    """FO_W6_XS=7 runs the X-stationary form on 7 waves x 4 code steps instead of 14 x 2 (the library reads the
    variable once per process, so this is a child process): one case of test_swiglu_k3584 under it."""
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                        f"{os.path.abspath(__file__)}::test_swiglu_k3584[16-176]"], env=dict(os.environ, FO_W6_XS="7"),
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True, text=True)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("chain", ["w6_w6swiglu", "w6_bf16", "bf16_w6"])
@pytest.mark.parametrize("M", [8, 16])
def test_rmsnorm_across_gemms(dev, M, chain):
    """The RMSNorm split across two GEMMs (tests/test_gemm_w4_gpu.py test_rmsnorm_across_gemms, its tolerances) with the
    MXFP6 GEMM as producer (+residual, yg, row sums), as consumer (rstd on the sums), or both."""
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
    _rose(before, w6=int(p6) + int(c6 and not sw), xs=int(sw))
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
    w, _ = _weight(100, 96, 200)
    lin = _lin(dev, w)
    x = torch.randn(16, 96, generator=torch.Generator().manual_seed(1)).to(dev)
    out = torch.full((16, 100), 7.0, device=dev)
    yg = torch.full((16, 100), 7.0, device=dev)
    st = ops.RowStats(16, dev)
    st.buf.fill_(-1.0)
    lin(x, out=out, M=3, stats_out=st.set(torch.ones(100, device=dev), yg))
    assert st.groups == 7
    assert (out[3:] == 7).all() and (yg[3:] == 7).all() and (st.buf[3 * 7:] == -1).all()
    assert torch.equal(out[:3], yg[:3])
    torch.testing.assert_close(st.buf[:21].view(3, 7).sum(1), (out[:3] ** 2).sum(1), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("M", [5, 16])
def test_long_k_split_form(dev, M):
    """The down projection's K with >= 16 tiles: 4 tiles per workgroup, K split across workgroups and merged in the
    launch.  272 columns are 17 tiles: the last group holds one tile of four.  Producer epilogue (+residual, yg, row
    sums) against float64; the tickets are left zeroed; repeated runs give equal bits."""
    from fo import ops
    N, K = 272, 18944
    w, wdq = _weight(N, K, 300)
    g = torch.Generator().manual_seed(M)
    x, r, gamma = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g), torch.rand(N, generator=g) + 0.5
    lin = _lin(dev, w)
    st = ops.RowStats(M, dev)
    runs = []
    before = _counts()
    for _ in range(2):
        out, yg = r.clone().to(dev), torch.zeros(M, N, device=dev)
        lin(x.to(dev), out=out, residual=True, stats_out=st.set(gamma.to(dev), yg))
        runs.append((out.cpu(), yg.cpu(), st.buf[:M * st.groups].cpu()))
    _rose(before, sk=2)
    assert st.groups == 17
    assert not ops.Runtime.get(dev).counters[:64].any()
    assert all(torch.equal(a, b) for a, b in zip(runs[1], runs[0]))
    ref = x.double() @ wdq.t() + r.double()
    torch.testing.assert_close(runs[0][0].double(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(runs[0][1].double(), ref * gamma.double(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(runs[0][2].view(M, 17).sum(1).double(), (ref * ref).sum(1), rtol=1e-4, atol=1e-4)


def test_17_rows_run_the_bf16_image(dev):
    from fo.ops import PackedLinear
    w, wdq = _weight(3584, 256, 100 + 3584)
    x = torch.randn(17, 256, generator=torch.Generator().manual_seed(17)).to(dev)
    lin = _lin(dev, w)
    before = _counts()
    y = lin(x)
    _rose(before)
    assert not lin.streams(17) and lin.streams(16)
    assert torch.equal(y, PackedLinear(wdq.to(torch.bfloat16).to(dev))(x))
    # ... and 16 rows of the same weight stream the codes: the same product to the kernels' accumulation order
    y16 = lin(x[:16])
    _rose(before, w6=1)
    torch.testing.assert_close(y16, y[:16], rtol=1e-4, atol=1e-4)
    # rows that are not fp32 run the image too
    xb = x[:16].to(torch.bfloat16)
    assert torch.equal(lin(xb), lin.bf16(xb))
    # a GEMM the policy keeps off the stream runs the image at every row count
    lin.stream = False
    assert not lin.streams(8) and torch.equal(lin(x[:16]), lin.bf16(x[:16]))
    _rose(before, w6=1)


@pytest.mark.parametrize("N", [80, 1000])
@pytest.mark.parametrize("M", [1, 16])
def test_head(dev, M, N):
    """fo_gemm_w6_head at K = 3584 against float64.  1000 columns are 63 tiles: an odd, ragged count whose last unit's
    second tile lies past both descriptors.  The 16-row output buffer is wider than N and filled with a sentinel: rows
    >= M and columns >= N keep it.  One head launch per call and no other counter moves; two runs are equal."""
    K = 3584
    w, wdq = _weight(N, K, 500 + N)
    lin = _lin(dev, w, kind="head")
    assert lin.ntiles == (N + 15) // 16 and lin.kind == "head"
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M + N))
    buf = torch.full((16, N + 5), -3.0, device=dev)
    before, others = _counts(), _others()
    y = lin(x.to(dev), out=buf[:, :N], M=M)
    _rose(before, head=1)
    assert _others() == others and y.data_ptr() == buf.data_ptr()
    got = buf.cpu()
    assert (got[M:] == -3).all() and (got[:, N:] == -3).all()
    torch.testing.assert_close(got[:M, :N].double(), x.double() @ wdq.t(), rtol=1e-4, atol=1e-4)
    again = torch.full((16, N + 5), -3.0, device=dev)
    lin(x.to(dev), out=again[:, :N], M=M)
    assert torch.equal(again, buf)


def test_head_policy_and_other_k(dev):
    """The constructor takes its dispatch from ops.W6_POLICY["head"] at K = 3584; a head of another K (the tiny config's
    128) streams through fo_gemm_w6's general plain form and never the head entry, which refuses that K by name."""
    from fo import _lib, ops
    w, _ = _weight(80, 3584, 580)
    assert ops.PackedLinearW6(w.to(dev), kind="head").stream == ops.W6_POLICY["head"]
    with pytest.raises(ValueError):
        ops.PackedLinearW6(w.to(dev), kind="attn_o")
    with pytest.raises(ValueError):
        ops.PackedLinearW6(w.to(dev), swiglu_up=w.to(dev), kind="head")
    g = torch.Generator().manual_seed(3)
    w, wdq = _weight(100, 128, 7)
    lin = ops.PackedLinearW6(w.to(dev), kind="head")
    assert lin.stream and lin.streams(16) and not lin.streams(17)
    x = torch.randn(5, 128, generator=g)
    before = _counts()
    y = lin(x.to(dev))
    _rose(before, w6=1)
    torch.testing.assert_close(y.cpu().double(), x.double() @ wdq.t(), rtol=1e-4, atol=1e-4)
    xd, out = x.to(dev), torch.empty(5, 100, device=dev)
    rc = _lib.load().fo_gemm_w6_head(xd.data_ptr(), 128, 5, 128, lin.q.data_ptr(), lin.scales.data_ptr(), lin.ntiles,
                                     100, out.data_ptr(), 100, None)
    assert rc == -2 and "fo_gemm_w6_head" in _lib.last_error() and "K=128" in _lib.last_error()
    _rose(before, w6=1)
