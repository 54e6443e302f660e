"""fo_quant_w8 / fo_gemm_w8 (weight-only FP8 for <= 16 rows): the device quantiser against the CPU reference bit for
bit, and the GEMM's epilogues against float64 on the DEQUANTISED weight -- the FP8 stream computes X . W'^T with the
bf16 kernels' arithmetic, so the tolerances are those of tests/test_gemm_gpu.py."""
import pytest
import torch

from gemm_w8_ref import _weight

pytestmark = pytest.mark.gpu


def _counts():
    from fo import ops
    c = ops.launch_counts()
    return c["gemm_w8"], c["gemm_w8_xs"]


def _edge_and_random():
    from test_quant_cpu import edge_weight
    g = torch.Generator().manual_seed(5)
    big = torch.randn(3584, 256, generator=g) * torch.exp(torch.randn(3584, 1, generator=g) * 3)
    return [edge_weight(), big.to(torch.bfloat16), big[:100, :96].contiguous()]   # (the last one fp32)


def test_quantiser_matches_the_cpu_reference(dev):
    from fo import ops
    from fo.quant import pack_codes, pack_scales, quantize_rows_e4m3
    for w in _edge_and_random():
        q, e, w_dq = quantize_rows_e4m3(w)
        qd, sd, dq = ops.quant_w8(w.to(dev))
        assert torch.equal(qd.cpu(), pack_codes(q)), tuple(w.shape)
        assert torch.equal(sd.cpu(), pack_scales(e)), tuple(w.shape)
        assert dq.dtype == torch.bfloat16 and torch.equal(dq.cpu().view(torch.int16), w_dq.view(torch.int16))
    # the SwiGLU pair: gate and up tiles interleaved
    from fo.ops import PackedLinearW8
    wg, wu = _edge_and_random()[0], _edge_and_random()[0].flip(0).contiguous()
    lin = PackedLinearW8(wg.to(dev), swiglu_up=wu.to(dev))
    (qg, eg, _), (qu, eu, _) = quantize_rows_e4m3(wg), quantize_rows_e4m3(wu)
    assert torch.equal(lin.q.cpu(), pack_codes(qu, 1, 2, pack_codes(qg, 0, 2, torch.zeros(lin.q.numel(), dtype=torch.uint8))))
    assert torch.equal(lin.scales.cpu(), pack_scales(eu, 1, 2, pack_scales(eg, 0, 2, torch.ones(lin.scales.numel()))))
    assert lin.fp8_nbytes == lin.q.numel() + 4 * lin.scales.numel() and lin.nbytes == lin.bf16.nbytes


@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (3, 100, 96), (16, 48, 18944), (8, 3584, 256)])
def test_plain_and_residual(dev, M, N, K):
    """(3, 100, 96): a ragged N and K % 64 == 32; (16, 48, 18944): the down projection's K."""
    from fo.ops import PackedLinearW8
    w, wdq = _weight(N, K, 100 + N)
    g = torch.Generator().manual_seed(M + K)
    x, r = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    lin = PackedLinearW8(w.to(dev))
    before = _counts()
    y = lin(x.to(dev))
    out = r.clone().to(dev)
    lin(x.to(dev), out=out, residual=True)
    assert _counts() == (before[0] + 2, before[1])
    ref = x.double() @ wdq.t()
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.cpu().double(), ref + r.double(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("N", [176, 4120])
@pytest.mark.parametrize("M", [1, 8, 16])
def test_swiglu_k3584(dev, M, N):
    """The X-stationary form; 4120 columns are 258 units: more than one per workgroup and a ragged last tile."""
    from fo.ops import PackedLinearW8
    K = 3584
    (wg, gdq), (wu, udq) = _weight(N, K, 1), _weight(N, K, 2)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M))
    lin = PackedLinearW8(wg.to(dev), swiglu_up=wu.to(dev))
    before = _counts()
    y = lin(x.to(dev))
    assert _counts() == (before[0], before[1] + 1)
    ref = torch.nn.functional.silu(x.double() @ gdq.t()) * (x.double() @ udq.t())
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_swiglu_general_form(dev):
    """The SwiGLU pair at another K (the tiny config's) runs the general form."""
    from fo.ops import PackedLinearW8
    M, N, K = 5, 200, 160
    (wg, gdq), (wu, udq) = _weight(N, K, 3), _weight(N, K, 4)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(9))
    before = _counts()
    y = PackedLinearW8(wg.to(dev), swiglu_up=wu.to(dev))(x.to(dev))
    assert _counts() == (before[0] + 1, before[1])
    ref = torch.nn.functional.silu(x.double() @ gdq.t()) * (x.double() @ udq.t())
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_swiglu_general_form_16_waves(dev):
    """34 code steps (K % 64 == 32): the SwiGLU pair on the general form's 16 waves."""
    from fo.ops import PackedLinearW8
    M, N, K = 5, 40, 2144
    (wg, gdq), (wu, udq) = _weight(N, K, 5), _weight(N, K, 6)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(9))
    before = _counts()
    y = PackedLinearW8(wg.to(dev), swiglu_up=wu.to(dev))(x.to(dev))
    assert _counts() == (before[0] + 1, before[1])
    ref = torch.nn.functional.silu(x.double() @ gdq.t()) * (x.double() @ udq.t())
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=1e-4)


def test_swiglu_k3584_other_wave_shape():
    """FO_W8_XS=8 runs the X-stationary form on 8 waves x 7 code steps instead of 14 x 4 (the library reads the
    variable once per process, so this is a child process): one case of test_swiglu_k3584 under it."""
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                        f"{os.path.abspath(__file__)}::test_swiglu_k3584[16-176]"], env=dict(os.environ, FO_W8_XS="8"),
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True, text=True)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("chain", ["w8_w8swiglu", "w8_bf16", "bf16_w8"])
@pytest.mark.parametrize("M", [8, 16])
def test_rmsnorm_across_gemms(dev, M, chain):
    """The RMSNorm split across two GEMMs (tests/test_gemm_gpu.py test_gemm_rmsnorm_across_gemms) with the FP8 GEMM as
    producer (+residual, yg, row sums), as consumer (rstd after the column scale), or both."""
    from fo import ops
    from fo.ops import PackedLinear, PackedLinearW8
    D = 3584
    g = torch.Generator().manual_seed(M)
    (wp, pdq), (wc, cdq), (wu, udq) = _weight(D, 1024, 20), _weight(4096, D, 21), _weight(4096, D, 22)
    gamma = torch.rand(D, generator=g) + 0.5
    xin, res = torch.randn(M, 1024, generator=g), torch.randn(M, D, generator=g)
    p8, c8, sw = chain.startswith("w8"), chain != "w8_bf16", chain == "w8_w8swiglu"
    prod = PackedLinearW8(wp.to(dev)) if p8 else PackedLinear(wp.to(dev))
    if c8:
        cons = PackedLinearW8(wc.to(dev), swiglu_up=wu.to(dev) if sw else None)
    else:
        cons = PackedLinear(wc.to(dev))
    st = ops.RowStats(M, dev)
    x = res.clone().to(dev)
    yg = torch.empty(M, D, device=dev)
    before = _counts()
    prod(xin.to(dev), out=x, residual=True, stats_out=st.set(gamma.to(dev), yg))
    out = cons(yg, norm=(st, 1e-6))
    after = _counts()
    assert after[0] - before[0] == int(p8) + int(c8 and not sw) and after[1] - before[1] == int(sw)
    y = res.double() + xin.double() @ (pdq if p8 else wp.double()).t()
    h = y * torch.rsqrt((y * y).mean(-1, keepdim=True) + 1e-6) * gamma.double()
    wcd = cdq if c8 else wc.double()
    ref = torch.nn.functional.silu(h @ wcd.t()) * (h @ udq.t()) if sw else h @ wcd.t()
    torch.testing.assert_close(x.cpu().double(), y, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(yg.cpu().double(), y * gamma.double(), rtol=1e-5, atol=1e-4)
    err = (out.cpu().double() - ref).abs().max().item()
    assert err < 2e-4 * ref.abs().max().item(), err


def test_17_rows_run_the_bf16_image(dev):
    from fo.ops import PackedLinear, PackedLinearW8
    w, wdq = _weight(3584, 256, 100 + 3584)
    x = torch.randn(17, 256, generator=torch.Generator().manual_seed(17)).to(dev)
    lin = PackedLinearW8(w.to(dev))
    before = _counts()
    y = lin(x)
    assert _counts() == before
    assert torch.equal(y, PackedLinear(wdq.to(torch.bfloat16).to(dev))(x))
    # ... and 16 rows of the same weight stream the codes: the same product to the kernels' accumulation order
    y16 = lin(x[:16])
    assert _counts() == (before[0] + 1, before[1])
    torch.testing.assert_close(y16, y[:16], rtol=1e-4, atol=1e-4)


def test_rows_beyond_m_are_not_written(dev):
    """Rows >= M are computed from a clamped row: never stored, never added into the row sums."""
    from fo import ops
    from fo.ops import PackedLinearW8
    w, _ = _weight(100, 96, 200)
    lin = PackedLinearW8(w.to(dev))
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
    """K >= 8192 with >= 16 tiles: 4 tiles per workgroup, K split across workgroups and merged in the launch.  272
    columns are 17 tiles: the last group holds one tile of four.  Producer epilogue (+residual, yg, row sums) against
    float64; the tickets are left zeroed; repeated runs give equal bits."""
    from fo import ops
    from fo.ops import PackedLinearW8
    N, K = 272, 8192
    w, wdq = _weight(N, K, 300)
    g = torch.Generator().manual_seed(M)
    x, r, gamma = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g), torch.rand(N, generator=g) + 0.5
    lin = PackedLinearW8(w.to(dev))
    st = ops.RowStats(M, dev)
    runs = []
    for _ in range(3):
        out, yg = r.clone().to(dev), torch.zeros(M, N, device=dev)
        lin(x.to(dev), out=out, residual=True, stats_out=st.set(gamma.to(dev), yg))
        runs.append((out.cpu(), yg.cpu(), st.buf[:M * st.groups].cpu()))
    assert st.groups == 17
    assert not ops.Runtime.get(dev).counters[:64].any()
    for o in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, runs[0]))
    ref = x.double() @ wdq.t() + r.double()
    torch.testing.assert_close(runs[0][0].double(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(runs[0][1].double(), ref * gamma.double(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(runs[0][2].view(M, 17).sum(1).double(), (ref * ref).sum(1), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(lin(x.to(dev)).cpu().double(), x.double() @ wdq.t(), rtol=1e-4, atol=1e-4)


def test_deterministic_down_shape(dev):
    from fo.ops import PackedLinearW8
    g = torch.Generator().manual_seed(3)
    M, N, K = 4, 3584, 18944
    lin = PackedLinearW8((torch.randn(N, K, generator=g) / 100).to(torch.bfloat16).to(dev))
    x = torch.randn(M, K, generator=g).to(dev)
    ys = [lin(x).cpu() for _ in range(5)]
    for y in ys[1:]:
        assert torch.equal(y, ys[0])
