"""The helper kernels of csrc/fo_elem.hip, fo_fbank (csrc/fo_audio.hip) and the silence cut (csrc/fo_codec.hip), each
launched alone through fo.ops between guards, against the float64 models of tests/helper_ref.py: bounded
operations within their derived bound, exact ones with torch.equal, and every byte a launch may not write
bit-identical afterwards.  tests/test_helper_ref_cpu.py shows that the bounds cannot hide a wrong kernel.

Observed max(err / bound) on an MI355X: rmsnorm 0.188 (float32 path; with round_fp16 every element equalled the model's
float32-exact value or its permitted neighbour), layernorm 0.131, fbank 0.071 (greatest log-domain bound 6.2e-4);
the silence cut's min_sum on the random rows equalled the model's float32 value (0 x 2^-23).
"""
import numpy as np
import pytest
import torch

import helper_ref as hr

pytestmark = pytest.mark.gpu
I32 = torch.int32


@pytest.fixture(scope="module")
def ops(dev):
    from fo import ops
    yield ops
    print("\nobserved max(err / bound):", {k: round(v, 4) for k, v in hr.OBSERVED.items()})


def _guarded(dev, t, ld=None):
    """t [M][D] inside a guard with row stride ld (guard columns hold the sentinel) -> (Guard, the [M][D] view)"""
    M, D = t.shape
    g = hr.Guard(dev, M, ld or D)
    g.t[:, :D] = t.to(dev)
    return g, g.t[:, :D]


# ================================================================================================ A. fo_elem.hip
@pytest.mark.parametrize("case", hr.RMS_CASES, ids=lambda c: c.name)
def test_rmsnorm_matches_float64(ops, dev, case):
    x, g = case.build()
    ref = hr.rmsnorm_ref(x, g, case.eps, case.rf)
    xb, xv = _guarded(dev, x, case.ldx)
    ob = xb if case.inplace else hr.Guard(dev, case.M, case.ldo)
    ob.mask[:, :case.D] = True
    gb, gv = _guarded(dev, g[None])
    for b in (xb, ob, gb):
        b.arm()
    ops.rmsnorm(xv, gv[0], case.eps, out=ob.t[:, :case.D], round_fp16=case.rf)
    torch.cuda.synchronize(dev)
    got = ob.check(case.name)[:, :case.D]
    xb.check(case.name + " x")
    gb.check(case.name + " w")
    r = hr.note("rmsnorm", hr.accept_rms(got, ref))
    print(f"{case.name}: max err/bound {r:.4f}")
    assert r <= 1.0
    if case.M == 3:
        assert bool((got[2] == 0).all())          # the all-zero row


@pytest.mark.parametrize("case", hr.LN_CASES, ids=lambda c: c.name)
def test_layernorm_matches_float64(ops, dev, case):
    x, w, b = case.build()
    y, E = hr.layernorm_ref(x, w, b, case.eps, case.act)
    xb, xv = _guarded(dev, x, case.ldx)
    ob = xb if case.inplace else hr.Guard(dev, case.M, case.ldo)
    ob.mask[:, :case.D] = True
    wb, wv = _guarded(dev, torch.stack([w, b]))
    for g in (xb, ob, wb):
        g.arm()
    ops.layernorm(xv, wv[0], wv[1], eps=case.eps, out=ob.t[:, :case.D], act=None if case.act == "none" else case.act)
    torch.cuda.synchronize(dev)
    got = ob.check(case.name)[:, :case.D]
    xb.check(case.name + " x")
    wb.check(case.name + " w, b")
    r = hr.note("layernorm", hr.ratio(got, y, E))
    print(f"{case.name}: max err/bound {r:.4f}")
    assert r <= 1.0
    # the constant row: the variance is exactly 0 and the output the activation of the bias, to the last bit
    want = {"none": b, "relu": torch.relu(b), "gelu": None}[case.act]
    if want is not None:
        assert torch.equal(got[1], want)


@pytest.mark.parametrize("case", hr.GATHER_CASES, ids=lambda c: c.name)
def test_gather_rows_is_exact(ops, dev, case):
    tab, idx, orow = case.build()
    D, M = case.D, case.M
    want = hr.gather_ref(tab, idx, M, D, case.rf)
    tb = hr.Guard(dev, *tab.shape, dtype=tab.dtype, fill=7.0)
    tb.t.copy_(tab)
    ld = case.col0 + D + 3
    ob = hr.Guard(dev, case.out_R, ld)
    rows = list(range(M)) if orow is None else orow.tolist()
    ob.mask[rows, case.col0:case.col0 + D] = True
    ob.arm()
    tb.arm()
    ops.gather_rows(tb.t[:, :D], None if idx is None else idx.to(dev), out=ob.t[:, case.col0:case.col0 + D],
                    round_fp16=case.rf, D=D, M=M, out_rows=None if orow is None else orow.to(dev))
    torch.cuda.synchronize(dev)
    got = ob.check(case.name)
    tb.check(case.name + " table")
    assert torch.equal(got[rows, case.col0:case.col0 + D], want)


@pytest.mark.parametrize("case", hr.STREAM_CASES, ids=lambda c: c.name)
def test_adapter_stream_state_is_exact(ops, dev, case):
    """Three consecutive chunks of two sessions through im2col_conv1d + conv_cache_update: every im2col row (pad
    columns zero) and the carried frames equal the model's, the slot pool's other rows stay untouched, and -- where
    the chunk length is a multiple of the stride -- the chunks' conv equals one float64 causal strided conv over the
    whole stream."""
    xs, w, model = hr.stream_model(case)
    B, KC, T, D, K, S = case.B, case.KC, case.T, case.D, case.K, case.S
    sel = case.slots or list(range(B))
    pool = hr.Guard(dev, case.pool, KC, D)
    pool.t[sel] = 0.0                                  # fresh sessions; the other rows keep the sentinel
    pool.mask[sel] = True
    slots = None if case.slots is None else torch.tensor(case.slots, dtype=I32, device=dev)
    cols_got = []
    for i, (x, (cols_want, cache_want)) in enumerate(zip(xs, model)):
        xb, _ = _guarded(dev, x.reshape(B * T, D))
        cols = hr.Guard(dev, *cols_want.shape)
        cols.mask[:] = True
        for g in (xb, cols, pool):
            g.arm()
        before = pool.full.clone()
        ops.im2col_conv1d(None if (i == 0 and case.null_first) else pool.t, slots, xb.t, B, KC, T, D, K, S, cols.t)
        torch.cuda.synchronize(dev)
        assert torch.equal(pool.full, before), "im2col_conv1d wrote the cache"
        got = cols.check(f"{case.name} chunk {i}")
        assert torch.equal(got, cols_want), f"chunk {i}: im2col"
        cols_got.append(got)
        ops.conv_cache_update(pool.t, slots, xb.t, B, KC, T, D)
        torch.cuda.synchronize(dev)
        assert torch.equal(pool.check(f"{case.name} chunk {i} pool")[sel], cache_want), f"chunk {i}: cache"
        xb.check(f"{case.name} chunk {i} x")
    if T % S == 0:
        assert hr.stream_property(case, xs, w, cols_got) <= 1.0


@pytest.mark.parametrize("n", [1, 257])
def test_scale_is_one_multiply(ops, dev, n):
    x = hr.randn(hr.gen(f"scale/{n}"), n)
    b = hr.Guard(dev, n)
    b.t.copy_(x)
    b.mask[:] = True
    b.arm()
    ops.scale_(b.t, hr.THIRD)
    torch.cuda.synchronize(dev)
    assert torch.equal(b.check("scale"), x * np.float32(hr.THIRD))


@pytest.mark.parametrize("case", hr.HASH_CASES, ids=lambda c: c.name)
def test_fill_hash_is_the_oracles_hash(ops, dev, case):
    dt = torch.bfloat16 if case.bf16 else torch.float32
    b = hr.Guard(dev, max(case.n, 4), dtype=dt)
    out = b.t[:case.n] if case.n else b.t[2:2]
    b.mask[:case.n] = True
    b.arm()
    ops.fill_hash(out, case.key, case.center, case.scale)
    torch.cuda.synchronize(dev)
    got = b.check(case.name)[:case.n]
    assert torch.equal(got.float(), hr.hash_ref(case.key, case.n, case.center, case.scale))


# ================================================================================================ B. fo_fbank
@pytest.mark.parametrize("case", hr.FBANK_CASES, ids=lambda c: c.name)
def test_fbank_matches_float64(ops, dev, case):
    d = case.build()
    wl, ws, nfft, window, twc, tws, mel = d.tables
    B, frames, row0, nmel = case.B, case.frames, case.row0, mel.shape[0]
    R = row0 + frames + 2
    out = hr.Guard(dev, B, R, nmel)
    out.mask[:, row0:row0 + frames] = True
    sb, sv = _guarded(dev, torch.from_numpy(d.samples))
    tabs = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (window, twc, tws, mel)]
    zr = None if case.zero_rows is None else torch.tensor(case.zero_rows, dtype=I32, device=dev)
    out.arm()
    sb.arm()
    ops.fbank(sv, B, d.n, wl, ws, nfft, *tabs, out.t.view(B, R * nmel), row0, zr)
    torch.cuda.synchronize(dev)
    got = out.check(case.name)[:, row0:row0 + frames].numpy()
    sb.check(case.name + " samples")
    if case.kind in ("zero", "dc"):
        # every mel energy is exactly 0: one value everywhere, the device's logf(FLT_EPSILON)
        v = float(got.flat[0])
        assert np.all(got == got.flat[0])
        assert abs(v - np.log(hr.FLT_EPS)) <= (hr.LOG_REL + hr.U) * abs(np.log(hr.FLT_EPS))
        return
    live = np.ones(got.shape, bool)
    for b, z in enumerate(case.zero_rows or []):
        live[b, :z] = False
        assert np.all(got[b, :z] == 0.0)               # zeroed frames are exactly 0
    assert np.isfinite(got).all()
    r = hr.note("fbank", float((np.abs(got.astype(np.float64) - d.want) / d.bound)[live].max()))
    print(f"{case.name}: max err/bound {r:.4f} (greatest bound {d.bound.max():.2e})")
    assert r <= 1.0


# ================================================================================================ C. silence cut
def _sil_buf(dev, x, ld=None):
    """rows of x inside zeros -- the guard elements and the padding between rows are the most attractive minimum, so
    any read past a row's L changes the answer"""
    x = np.atleast_2d(x)
    b = hr.Guard(dev, x.shape[0], ld or x.shape[1], fill=0.0)
    b.t[:, :x.shape[1]] = torch.from_numpy(x).to(dev)
    return b, b.t[:, :x.shape[1]]


def _sil_want(x, N):
    ms, cut = hr.silence_ref(x, N)
    return torch.tensor([ms, np.float32(cut)], dtype=torch.float32)


@pytest.mark.parametrize("case", hr.SIL_EXACT, ids=lambda c: c.name)
def test_silence_cut_exact_rows(ops, dev, case):
    x = case.build()
    xb, xv = _sil_buf(dev, x)
    res = hr.Guard(dev, 2)
    res.mask[:] = True
    res.arm()
    xb.arm()
    ops.silence_cut(xv[0], case.N, res.t)
    torch.cuda.synchronize(dev)
    got = res.check(case.name)
    xb.check(case.name + " x")
    want = _sil_want(x, case.N)
    print(f"{case.name}: (min_sum, cut) {got.tolist()} model {want.tolist()}")
    assert torch.equal(got.view(I32), want.view(I32))


def test_silence_cut_rows_equal_single_rows(ops, dev):
    c = hr.SIL_ROWS
    rows = c.build()
    xb, xv = _sil_buf(dev, rows, c.ld)
    res = hr.Guard(dev, rows.shape[0], 2)
    res.mask[:] = True
    res.arm()
    xb.arm()
    ops.silence_cut_rows(xv, c.N, res.t)
    torch.cuda.synchronize(dev)
    got = res.check(c.name)
    xb.check(c.name + " x")
    for r in range(rows.shape[0]):
        one = ops.silence_cut(xv[r].contiguous(), c.N, torch.empty(2, device=dev)).cpu()
        assert torch.equal(got[r].view(I32), _sil_want(rows[r], c.N).view(I32)), r
        assert torch.equal(got[r].view(I32), one.view(I32)), r


@pytest.mark.parametrize("case", hr.SIL_RANDOM, ids=lambda c: c.name)
def test_silence_cut_random_rows(ops, dev, case):
    x = case.build()
    xb, xv = _sil_buf(dev, x)
    res = hr.Guard(dev, 2)
    res.mask[:] = True
    res.arm()
    ops.silence_cut(xv[0], case.N, res.t)
    torch.cuda.synchronize(dev)
    got = res.check(case.name)
    ms, cut = hr.silence_ref(x, case.N)
    rel = abs(float(got[0]) - float(ms)) / float(ms)
    print(f"{case.name}: cut {int(got[1])} model {cut}, min_sum off by {rel / 2.0 ** -23:.3f} x 2^-23")
    assert int(got[1]) == cut
    assert rel <= 2.0 ** -23
