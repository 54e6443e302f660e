"""The codec encoder's kernels (csrc/fo_codec_enc.hip: conv1d_ex, group_norm, gte_head, vq_nearest), each launched
alone through fo.ops between guards, against the float64 models of tests/helper_ref.py -- the real geometry (a
1024-code book of width 512) included: outputs within their derived bound, code ids and the straight-through residual
exact, ties to the lowest index, and every byte a launch may not write bit-identical afterwards.
tests/test_helper_ref_cpu.py shows that the bounds cannot hide a wrong kernel and that every row's best code is
clear of the float32 error.

Observed max(err / bound) on an MI355X: conv1d_ex 0.536 (Cin = K = 1, where the bound is four roundings), group_norm
0.125, gte_head 0.049; the least VQ gap was 1874 times twice the float32 error.
"""
import numpy as np
import pytest
import torch

import helper_ref as hr

pytestmark = pytest.mark.gpu
I32 = torch.int32
FAM = ("conv1d_ex", "group_norm", "gte_head")


@pytest.fixture(scope="module")
def ops(dev):
    from fo import ops
    yield ops
    print("\nobserved max(err / bound):", {k: round(v, 4) for k, v in hr.OBSERVED.items() if k in FAM})


def _inp(dev, *ts):
    """read-only inputs, each inside its own armed guard -> (guards, device views)"""
    gs = []
    for t in ts:
        g = hr.Guard(dev, *t.shape, dtype=t.dtype)
        g.t.copy_(t)
        gs.append(g.arm())
    return gs, [g.t for g in gs]


def _untouched(gs, what):
    for i, g in enumerate(gs):
        g.check(f"{what} input {i}")


@pytest.mark.parametrize("case", hr.CONVEX_CASES, ids=lambda c: c.name)
def test_conv1d_ex_matches_float64(ops, dev, case):
    d = case.build()
    y, E = hr.conv_ex_ref(d.x, d.w, d.bias, case.stride, case.dil, case.pad, case.slope, d.prefill)
    gs, (x, w) = _inp(dev, d.x, d.w)
    bias = None
    if d.bias is not None:
        gb, (bias,) = _inp(dev, d.bias)
        gs += gb
    out = hr.Guard(dev, case.B, case.Cout, case.Tout)
    if case.residual:
        out.t.copy_(d.prefill)
    out.mask[:] = True
    out.arm()
    ops.conv1d_ex(x, case.B, case.Cin, case.Tin, w, bias, case.Cout, case.K, case.stride, case.dil, case.pad,
                  case.slope, out.t, residual=case.residual)
    torch.cuda.synchronize(dev)
    got = out.check(case.name)
    _untouched(gs, case.name)
    r = hr.note("conv1d_ex", hr.ratio(got, y, E))
    print(f"{case.name}: max err/bound {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("case", hr.GN_CASES, ids=lambda c: c.name)
def test_group_norm_matches_float64(ops, dev, case):
    x, w, b = case.build()
    y, E = hr.group_norm_ref(x, case.G, w, b, case.eps, case.scale)
    gs, (xd, wd, bd) = _inp(dev, x, w, b)
    out = gs[0] if case.inplace else hr.Guard(dev, *x.shape)
    out.mask[:] = True
    out.arm()
    ops.group_norm(xd, case.B, case.C, case.T, case.G, wd, bd, case.eps, case.scale, out.t)
    torch.cuda.synchronize(dev)
    got = out.check(case.name)
    _untouched(gs[1:] if case.inplace else gs, case.name)
    r = hr.note("group_norm", hr.ratio(got, y, E))
    print(f"{case.name}: max err/bound {r:.4f}")
    assert r <= 1.0
    # the constant group: exactly bias * scale
    assert torch.equal(got[1, :16], (b[:16] * np.float32(case.scale))[:, None].expand(16, case.T))


@pytest.mark.parametrize("case", hr.GTE_CASES, ids=lambda c: c.name)
def test_gte_head_matches_float64(ops, dev, case):
    d = case.build()
    y, E = hr.gte_ref(d.x, d.lw, d.lb, d.rm, d.rv, d.bw, d.bb, case.eps)
    gs, dv = _inp(dev, d.x, d.lw, d.lb, d.rm, d.rv, d.bw, d.bb)
    out = hr.Guard(dev, case.B, case.C)
    out.mask[:] = True
    out.arm()
    ops.gte_head(dv[0], case.B, case.C, case.T, *dv[1:], case.eps, out.t)
    torch.cuda.synchronize(dev)
    got = out.check(case.name)
    _untouched(gs, case.name)
    r = hr.note("gte_head", hr.ratio(got, y, E))
    print(f"{case.name}: max err/bound {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("case", hr.VQ_CASES, ids=lambda c: c.name)
def test_vq_nearest_ids_and_residual_are_exact(ops, dev, case):
    d = case.build()
    B, T, D, ch0 = d.B, case.T, case.D, d.ch0
    want_ids, gap, err = hr.vq_ref(d.rows, d.E)
    (xg, eg), (x, E) = _inp(dev, d.x, d.E)
    xg.mask[:, ch0:ch0 + D] = case.residual
    ids = hr.Guard(dev, B * T, case.ids_ld, dtype=I32)
    ids.mask[:, case.ids_col] = True
    ids.arm()
    ops.vq_nearest(x, B, d.Ctot, T, ch0, D, E, ids.t, case.ids_ld, case.ids_col, residual=case.residual)
    torch.cuda.synchronize(dev)
    got_ids = ids.check(case.name + " ids")[:, case.ids_col]
    got_x = xg.check(case.name + " x")
    eg.check(case.name + " codebook")
    print(f"{case.name}: least gap / (2 err) {float((gap / (2 * err)).min()):.1f}")
    assert torch.equal(got_ids, want_ids), (got_ids.tolist(), want_ids.tolist())
    if case.residual:
        want = hr.vq_residual32(d.rows, d.E[want_ids.long()]).reshape(B, T, D).transpose(1, 2)
        assert torch.equal(got_x[:, ch0:ch0 + D], want)
