"""fo_quant_w4 / fo_gemm_w4 (weight-only MXFP4 for <= 16 rows): the device quantiser against the CPU definition bit for
bit, and every form and epilogue of the GEMM against float64 X . W'^T on the CPU definition's W' -- the MXFP4 stream
decodes the codes to the exact bf16 W' and runs the bf16 kernels' arithmetic, so the tolerances are those of
tests/test_gemm_gpu.py (rtol = atol = 1e-4), as for the FP8 stream."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _weight(N, K, seed, block_scaled=False):
    """(bf16 weight, its dequantised MXFP4 image as float64), on the CPU, shared between the tests.  block_scaled:
    block j of every row times 2^-(j mod 7), so that a kernel applying another block's scale is far off (magnitudes
    only shrink: the tolerance keeps its meaning)."""
    from fo.quant import quantize_blocks_e2m1
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    if block_scaled:
        w = w * (2.0 ** -(torch.arange(K // 32) % 7).float()).repeat_interleave(32)[None]
    w = w.to(torch.bfloat16)
    return w, quantize_blocks_e2m1(w)[2].double()


@functools.lru_cache(maxsize=None)
def _swiglu_ref(N, K, M):
    (_, gdq), (_, udq) = _weight(N, K, 1), _weight(N, K, 2)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M))
    return x, torch.nn.functional.silu(x.double() @ gdq.t()) * (x.double() @ udq.t())


def _lin(dev, w, up=None):
    """PackedLinearW4 that streams the codes at <= 16 rows whatever the measured dispatch policy keeps on the image."""
    from fo.ops import PackedLinearW4
    p = PackedLinearW4(w.to(dev), swiglu_up=None if up is None else up.to(dev))
    p.stream = True
    return p


def _counts():
    from fo import ops
    c = ops.w4_launch_counts()
    return c["w4"], c["w4_xs"], c["w4_sk"]


def _rose(before, w4=0, xs=0, sk=0):
    assert _counts() == (before[0] + w4, before[1] + xs, before[2] + sk)


def test_quantiser_matches_the_cpu_definition(dev):
    from fo import ops
    from fo.quant import pack_codes_w4, pack_scales_w4, quantize_blocks_e2m1
    from test_quant_w4_cpu import edge_weight_w4
    g = torch.Generator().manual_seed(5)
    big = torch.randn(3584, 256, generator=g) * torch.exp(torch.randn(3584, 8, generator=g) * 3).repeat_interleave(32, 1)
    for w in (edge_weight_w4(), big.to(torch.bfloat16), big[:100, :96].contiguous()):   # (the last one fp32)
        q, e, w_dq = quantize_blocks_e2m1(w)
        for base, stride in ((0, 1), (1, 2)):
            qd, sd, dq = ops.quant_w4(w.to(dev), base, stride)
            assert torch.equal(qd.cpu(), pack_codes_w4(q, base, stride)), (tuple(w.shape), base)
            assert torch.equal(sd.cpu(), pack_scales_w4(e, base, stride)), (tuple(w.shape), base)
            assert dq.dtype == torch.bfloat16 and torch.equal(dq.cpu().view(torch.int16), w_dq.view(torch.int16))
    # the SwiGLU pair: gate and up tiles interleaved
    from fo.ops import PackedLinearW4
    wg, wu = edge_weight_w4(), edge_weight_w4().flip(0).contiguous()
    lin = PackedLinearW4(wg.to(dev), swiglu_up=wu.to(dev))
    (qg, eg, _), (qu, eu, _) = quantize_blocks_e2m1(wg), quantize_blocks_e2m1(wu)
    assert torch.equal(lin.q.cpu(), pack_codes_w4(qu, 1, 2, pack_codes_w4(qg, 0, 2, torch.zeros(lin.q.numel(), dtype=torch.uint8))))
    assert torch.equal(lin.scales.cpu(),
                       pack_scales_w4(eu, 1, 2, pack_scales_w4(eg, 0, 2, torch.zeros(lin.scales.numel(), dtype=torch.uint8))))
    assert lin.fp4_nbytes == lin.q.numel() + lin.scales.numel() and lin.nbytes == lin.bf16.nbytes


@pytest.mark.parametrize("block_scaled", [False, True])
@pytest.mark.parametrize("M,N,K", [(1, 64, 128), (3, 100, 96), (16, 48, 18944), (8, 3584, 256)])
def test_plain_and_residual(dev, M, N, K, block_scaled):
    """(3, 100, 96): a ragged N and K % 128 == 96; (16, 48, 18944): the down projection's K.  The hardware convert's
    nibble order and the block-scale indexing both show here: W' is the CPU definition's."""
    w, wdq = _weight(N, K, 100 + N, block_scaled)
    g = torch.Generator().manual_seed(M + K)
    x, r = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    lin = _lin(dev, w)
    before = _counts()
    y = lin(x.to(dev))
    out = r.clone().to(dev)
    lin(x.to(dev), out=out, residual=True)
    _rose(before, w4=2)
    ref = x.double() @ wdq.t()
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.cpu().double(), ref + r.double(), rtol=1e-4, atol=1e-4)


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
    _rose(before, w4=1)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_swiglu_general_form_16_waves(dev):
    """17 code steps (K % 128 == 96): the SwiGLU pair on the general form's 16 waves."""
    M, N, K = 5, 40, 2144
    x, ref = _swiglu_ref(N, K, M)
    lin = _lin(dev, _weight(N, K, 1)[0], _weight(N, K, 2)[0])
    before = _counts()
    y = lin(x.to(dev))
    _rose(before, w4=1)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_swiglu_k3584_other_wave_shape():
    """FO_W4_XS=7 runs the X-stationary form on 7 waves x 4 code steps instead of 14 x 2 (the library reads the
    variable once per process, so this is a child process): one case of test_swiglu_k3584 under it."""
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                        f"{os.path.abspath(__file__)}::test_swiglu_k3584[16-176]"], env=dict(os.environ, FO_W4_XS="7"),
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True, text=True)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("chain", ["w4_w4swiglu", "w4_bf16", "bf16_w4"])
@pytest.mark.parametrize("M", [8, 16])
def test_rmsnorm_across_gemms(dev, M, chain):
    """The RMSNorm split across two GEMMs (tests/test_gemm_w8_gpu.py test_rmsnorm_across_gemms, its tolerances) with the
    MXFP4 GEMM as producer (+residual, yg, row sums), as consumer (rstd on the sums), or both."""
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
    _rose(before, w4=int(p4) + int(c4 and not sw), xs=int(sw))
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
    for _ in range(3):
        out, yg = r.clone().to(dev), torch.zeros(M, N, device=dev)
        lin(x.to(dev), out=out, residual=True, stats_out=st.set(gamma.to(dev), yg))
        runs.append((out.cpu(), yg.cpu(), st.buf[:M * st.groups].cpu()))
    _rose(before, sk=3)
    assert st.groups == 17
    assert not ops.Runtime.get(dev).counters[:64].any()
    for o in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, runs[0]))
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
    assert torch.equal(y, PackedLinear(wdq.to(torch.bfloat16).to(dev))(x))
    # ... and 16 rows of the same weight stream the codes: the same product to the kernels' accumulation order
    y16 = lin(x[:16])
    _rose(before, w4=1)
    torch.testing.assert_close(y16, y[:16], rtol=1e-4, atol=1e-4)
    # a GEMM the policy keeps off the stream runs the image at every row count
    lin.stream = False
    assert not lin.streams(8) and torch.equal(lin(x[:16]), lin.bf16(x[:16]))
    _rose(before, w4=1)
