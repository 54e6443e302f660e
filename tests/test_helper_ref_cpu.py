"""tests/helper_ref.py on the CPU: every condition its case tables rest on holds from the models alone (ambiguous
fp16 roundings, the fbank bound's ceiling, silence-cut and VQ margins), each listed mutant of a model leaves the
bound or changes an exact result on at least one table case, a plain float32 restatement of each bounded kernel stays
inside its bound (so the bounds are not out of a correct kernel's reach), and the host-side refusals added with
them: fo_rmsnorm's alignment check and the layout asserts of ops.im2col_conv1d / ops.conv_cache_update."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helper_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("FO_LIB_PATH") or os.path.join(ROOT, "freeze-omni_amd", "fo", "libfo_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libfo_hip.so not built (run __graft_entry__.build())")
FAKE = 1 << 20   # dummy device address: never dereferenced by a refused call


def _over(got, y, E):
    """a mutant's output, rounded to float32 like a kernel's, leaves the bound (or is not finite)"""
    got = got.float()
    return (not bool(torch.isfinite(got).all())) or hr.ratio(got, y, E) > 1.0


# ------------------------------------------------------------------------------------------------ conditions
@pytest.mark.parametrize("case", [c for c in hr.RMS_CASES if c.rf], ids=lambda c: c.name)
def test_rmsnorm_ambiguous_fp16_share(case):
    x, g = case.build()
    ref = hr.rmsnorm_ref(x, g, case.eps, True)
    share = float(ref.amb.double().mean())
    print(f"{case.name}: {100 * share:.3f} % of the elements may round to the neighbouring fp16 value")
    assert share <= 0.01
    assert bool((ref.alt != ref.exact)[ref.amb].all())


_FB = {}


def _fb(case):
    if case.name not in _FB:
        _FB[case.name] = case.build()
    return _FB[case.name]


@pytest.mark.parametrize("case", hr.FBANK_CASES, ids=lambda c: c.name)
def test_fbank_bound_ceiling(case):
    d = _fb(case)
    if case.kind in ("zero", "dc"):
        assert np.all(d.want == np.log(hr.FLT_EPS))      # every mel energy is exactly 0 in the model
        return
    print(f"{case.name}: greatest log-domain bound {d.bound.max():.3e}")
    assert d.bound.max() < hr.FB_CEIL
    if case.kind == "faint":
        e = np.exp(d.want)
        assert (e < 4 * hr.FLT_EPS).any() and (e > hr.FLT_EPS).any()


def test_fft_model_is_a_dft():
    wl, ws, nfft, window, twc, tws, mel = hr.fbank_tables("A")
    y = np.random.default_rng(0).standard_normal((3, nfft))
    k = np.arange(nfft // 2)
    re, im = hr.fft_tables64(y, np.cos(2 * np.pi * k / nfft), np.sin(2 * np.pi * k / nfft))
    want = np.fft.fft(y)
    assert np.abs(re + 1j * im - want).max() < 1e-11


@pytest.mark.parametrize("case", hr.SIL_EXACT + [hr.SIL_ROWS], ids=lambda c: c.name)
def test_silence_exact_rows_are_exact(case):
    x = case.build()
    if case.name.startswith("cast-tie"):
        return
    assert np.all(x * 64 == np.round(x * 64)) and np.abs(x).max() < 4


@pytest.mark.parametrize("case", hr.SIL_RANDOM, ids=lambda c: c.name)
def test_silence_random_rows_have_a_clear_minimum(case):
    gap = hr.silence_gap_ulps(case.build(), case.N)
    print(f"{case.name}: runner-up {gap:.0f} float ulps above the best window")
    assert gap >= 4


@pytest.mark.parametrize("case", hr.VQ_CASES, ids=lambda c: c.name)
def test_vq_gap_condition(case):
    d = case.build()
    ids, gap, err = hr.vq_ref(d.rows, d.E)
    if case.n_codes > 1:
        print(f"{case.name}: least gap / (2 err) {float((gap / (2 * err)).min()):.1f}")
        assert bool((gap > 2 * err).all())
    # a row built on a duplicated code picks the pair's lower index
    lower = {hi: lo for lo, hi in case.dups}
    want = torch.tensor([lower.get(int(t), int(t)) for t in d.tgt], dtype=torch.int32)
    assert torch.equal(ids, want)


def test_hash_model_is_the_oracles():
    from oracle import weights as ow
    got = hr.hash_ref(ow.tensor_key(5, "a.weight"), 1000, 0.25, 0.5)
    assert np.array_equal(got.numpy(), ow.hash_uniform(5, "a.weight", (1000,), 0.25, 0.5))


# ------------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize("mut", ["noeps", "nm1", "gshift", "nofp16", "fp16late"])
def test_rmsnorm_mutants_are_rejected(mut):
    hit = []
    for c in hr.RMS_CASES:
        if mut in ("nofp16", "fp16late") and not c.rf:
            continue
        x, g = c.build()
        ref = hr.rmsnorm_ref(x, g, c.eps, c.rf)
        assert hr.accept_rms(ref.y.float(), ref) <= 1.0            # the model's own output passes
        if hr.accept_rms(hr.rmsnorm_ref(x, g, c.eps, c.rf, (mut,)).y.float(), ref) > 1.0:
            hit.append(c.name)
    assert hit, mut


@pytest.mark.parametrize("mut", ["unbiased", "onepass", "actfirst", "tanh"])
def test_layernorm_mutants_are_rejected(mut):
    hit = []
    for c in hr.LN_CASES:
        x, w, b = c.build()
        y, E = hr.layernorm_ref(x, w, b, c.eps, c.act)
        if _over(hr.layernorm_ref(x, w, b, c.eps, c.act, (mut,))[0], y, E):
            hit.append(c.name)
    print(mut, hit)
    assert hit, mut
    if mut == "onepass":
        assert any("none" in n or "relu" in n or "gelu" in n for n in hit)


@pytest.mark.parametrize("mut", ["colorder", "cacheshift", "nostride", "first"])
def test_stream_mutants_change_an_exact_result(mut):
    hit = 0
    for c in hr.STREAM_CASES:
        _, _, good = hr.stream_model(c)
        _, _, bad = hr.stream_model(c, mut_im=() if mut == "first" else (mut,), mut_cache=(mut,) if mut == "first" else ())
        hit += any(not torch.equal(a[0], b[0]) or not torch.equal(a[1], b[1]) for a, b in zip(good, bad))
    assert hit, mut


@pytest.mark.parametrize("case", hr.STREAM_CASES, ids=lambda c: c.name)
def test_stream_chunks_equal_one_conv_over_the_stream(case):
    xs, w, out = hr.stream_model(case)
    r = hr.stream_property(case, xs, w, [c for c, _ in out])
    if case.T % case.S == 0:
        assert r <= 1.0
    else:
        assert r > 1.0     # an odd chunk under stride 2 restarts the stride's phase (the reference does too)


@pytest.mark.parametrize("mut", ["nomean", "pre0", "hann", "logadd", "melshift"])
def test_fbank_mutants_are_rejected(mut):
    hit = []
    for c in hr.FBANK_CASES:
        if c.kind in ("zero", "dc"):
            continue
        d = _fb(c)
        wl, ws, nfft, window, twc, tws, mel = d.tables
        bad, _ = hr.fbank_ref(d.samples, d.n, wl, ws, nfft, window, twc, tws, mel, (mut,))
        if np.any(np.abs(bad.astype(np.float32) - d.want) > d.bound):
            hit.append(c.name)
    print(mut, hit)
    assert hit, mut


@pytest.mark.parametrize("mut", ["last", "e0", "mid", "double"])
def test_silence_mutants_change_an_exact_result(mut):
    hit = []
    for c in hr.SIL_EXACT:
        x = c.build()
        if hr.silence_ref(x, c.N) != hr.silence_ref(x, c.N, (mut,)):
            hit.append(c.name)
    print(mut, hit)
    assert hit, mut
    if mut == "double":
        assert hit == ["cast-tie/L9/N4"]


def test_silence_model_on_the_documented_cases():
    by = {c.name: c for c in hr.SIL_EXACT}
    assert hr.silence_ref(by["cast-tie/L9/N4"].build(), 4) == (np.float32(1201.0), 2)
    z = by["zeros/L4097/N2401"]
    assert hr.silence_ref(z.build(), z.N) == (np.float32(0.0), 4097 // 2 - 2401 // 2)
    b = by["L36863/N2401/unstaged"].build()
    for name, L in (("L36798/N2401/staged", 36798), ("L36799/N2401/unstaged", 36799), ("L36862/N2401/unstaged", 36862)):
        assert np.array_equal(by[name].build(), b[:L])      # one prefix, staged and unstaged
    assert hr.SC_MAX_STAGE == 36798
    c = by["argmin/L6000/N2401"]
    st = 3000 - 1200
    assert hr.silence_ref(c.build(), c.N)[1] == st + 10 + 5
    rows = hr.SIL_ROWS.build()
    assert np.abs(rows).min() > 0      # the zero padding between rows is the most attractive minimum


@pytest.mark.parametrize("mut", ["flip", "dilstride"])
def test_conv_ex_mutants_are_rejected(mut):
    hit = []
    for c in hr.CONVEX_CASES:
        d = c.build()
        y, E = hr.conv_ex_ref(d.x, d.w, d.bias, c.stride, c.dil, c.pad, c.slope, d.prefill)
        assert y.shape[2] == c.Tout
        if _over(hr.conv_ex_ref(d.x, d.w, d.bias, c.stride, c.dil, c.pad, c.slope, d.prefill, (mut,))[0], y, E):
            hit.append(c.name)
    assert hit, mut


def test_group_norm_and_gte_mutants_are_rejected():
    hit = []
    for c in hr.GN_CASES:
        x, w, b = c.build()
        y, E = hr.group_norm_ref(x, c.G, w, b, c.eps, c.scale)
        if _over(hr.group_norm_ref(x, c.G, w, b, c.eps, c.scale, ("perchannel",))[0], y, E):
            hit.append(c.name)
    assert hit
    hit = []
    for c in hr.GTE_CASES:
        d = c.build()
        a = (d.x, d.lw, d.lb, d.rm, d.rv, d.bw, d.bb, c.eps)
        y, E = hr.gte_ref(*a)
        if _over(hr.gte_ref(*a, ("leakylast",))[0], y, E):
            hit.append(c.name)
    assert hit


@pytest.mark.parametrize("mut", ["last", "noee"])
def test_vq_mutants_change_the_ids(mut):
    hit = []
    for c in hr.VQ_CASES:
        d = c.build()
        if not torch.equal(hr.vq_ref(d.rows, d.E)[0], hr.vq_ref(d.rows, d.E, (mut,))[0]):
            hit.append(c.name)
    print(mut, hit)
    assert hit, mut


# ------------------------------------------------------------------------------------------------ float32 stand-ins
def test_float32_restatements_stay_inside_the_bounds():
    """Each bounded operation again in plain float32 torch (another summation order than the kernel's, the same
    number formats): inside the bound with room to spare, so a correct kernel is not out of its reach."""
    worst = {}

    def up(k, r):
        worst[k] = max(worst.get(k, 0.0), r)
    for c in hr.RMS_CASES:
        x, g = c.build()
        r = torch.rsqrt((x * x).sum(-1, keepdim=True) / c.D + np.float32(c.eps))
        h = x * r
        up("rms", hr.accept_rms(g * (h.half().float() if c.rf else h), hr.rmsnorm_ref(x, g, c.eps, c.rf)))
    for c in hr.LN_CASES:
        x, w, b = c.build()
        y, E = hr.layernorm_ref(x, w, b, c.eps, c.act)
        m = x.mean(-1, keepdim=True)
        v = ((x - m) ** 2).mean(-1, keepdim=True)
        o = (x - m) * (1.0 / torch.sqrt(v + np.float32(c.eps))) * w + b
        o = {"none": o, "relu": torch.relu(o), "gelu": F.gelu(o)}[c.act]
        up("ln", hr.ratio(o, y, E))
    for c in hr.GN_CASES:
        x, w, b = c.build()
        y, E = hr.group_norm_ref(x, c.G, w, b, c.eps, c.scale)
        up("gn", hr.ratio(F.group_norm(x, c.G, w, b, c.eps) * np.float32(c.scale), y, E))
    for c in hr.CONVEX_CASES:
        d = c.build()
        y, E = hr.conv_ex_ref(d.x, d.w, d.bias, c.stride, c.dil, c.pad, c.slope, d.prefill)
        xa = d.x if c.slope is None else torch.where(d.x < 0, d.x * np.float32(c.slope), d.x)
        o = F.conv1d(xa, d.w, d.bias, stride=c.stride, dilation=c.dil, padding=c.pad)
        up("conv", hr.ratio(o if d.prefill is None else d.prefill + o, y, E))
    for c in hr.GTE_CASES:
        d = c.build()
        y, E = hr.gte_ref(d.x, d.lw, d.lb, d.rm, d.rv, d.bw, d.bb, c.eps)
        v = torch.where(d.x < 0, d.x * np.float32(0.1), d.x).mean(-1)
        t = v @ d.lw.t() + d.lb
        t = torch.where(t < 0, t * np.float32(0.1), t)
        up("gte", hr.ratio((t - d.rm) * torch.rsqrt(d.rv + np.float32(c.eps)) * d.bw + d.bb, y, E))
    print({k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("case", [c for c in hr.FBANK_CASES if c.kind in ("signal", "faint")][:4], ids=lambda c: c.name)
def test_float32_fbank_stays_inside_the_bound(case):
    d = _fb(case)
    wl, ws, nfft, window, twc, tws, mel = d.tables
    f32 = np.float32
    x = d.samples[:, :d.n]
    frames = 1 + (d.n - wl) // ws
    fr = np.stack([x[:, f * ws:f * ws + wl] for f in range(frames)], 1)
    mean = (fr.sum(-1, keepdims=True, dtype=f32) / f32(wl)).astype(f32)
    xi = fr - mean
    prev = np.concatenate([fr[..., :1], fr[..., :-1]], -1) - mean
    y = np.zeros(fr.shape[:2] + (nfft,), f32)
    y[..., :wl] = (xi - f32(0.97) * prev) * window
    re, im = hr.fft_tables64(y, twc, tws)
    assert re.dtype == f32
    e = ((re * re + im * im)[..., :nfft // 2 + 1] @ mel.T).astype(f32)
    got = np.log(np.maximum(e, f32(hr.FLT_EPS)))
    r = float((np.abs(got.astype(np.float64) - d.want) / d.bound).max())
    print(f"{case.name}: float32 restatement err / bound {r:.4f}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------ host-side refusals
@needs_lib
def test_rmsnorm_refuses_unaligned_pointers():
    from fo import _lib
    import ctypes
    lib, err = _lib.load(), _lib.last_error
    eps = ctypes.c_float(1e-6)

    def call(x, w, out, D=8, ldx=8, ldo=8):
        return lib.fo_rmsnorm(x, ldx, 1, D, w, eps, out, ldo, 0, None)
    for bad in ((FAKE + 4, FAKE, FAKE), (FAKE, FAKE + 8, FAKE), (FAKE, FAKE, FAKE + 12), (FAKE, None, FAKE)):
        assert call(*bad) == -2 and "16-byte aligned" in err(), (bad, err())
    assert call(FAKE, FAKE, FAKE, D=6) == -2 and "bad shape" in err()
    assert call(FAKE, FAKE, FAKE, ldx=10) == -2 and "bad shape" in err()


@needs_lib
def test_fill_hash_of_nothing_launches_nothing():
    from fo import _lib
    import ctypes
    lib = _lib.load()
    for out in (FAKE, None):          # an empty tensor's address is null
        assert lib.fo_fill_hash(out, 0, 0, 7, ctypes.c_float(0.0), ctypes.c_float(1.0), None) == 0
    assert lib.fo_fill_hash(None, 0, 1, 7, ctypes.c_float(0.0), ctypes.c_float(1.0), None) == -2


def test_stream_wrappers_assert_their_layout():
    from fo import ops
    B, KC, T, D, K = 2, 2, 4, 3, 3
    x, cache, out = torch.zeros(B * T, D), torch.zeros(B, KC, D), torch.zeros(B * 2, D * K)
    wide = torch.zeros(B * T, D + 1)
    for bad_x in (wide[:, :D], wide, torch.zeros(B * T - 1, D), x.double()):
        with pytest.raises(AssertionError, match="x "):
            ops.im2col_conv1d(cache, None, bad_x, B, KC, T, D, K, 2, out)
        with pytest.raises(AssertionError, match="x "):
            ops.conv_cache_update(cache, None, bad_x, B, KC, T, D)
    for bad_c in (torch.zeros(B, KC, D + 1)[:, :, :D], torch.zeros(B, KC + 1, D), torch.zeros(B - 1, KC, D),
                  torch.zeros(B * KC, D)):
        with pytest.raises(AssertionError, match="cache "):
            ops.im2col_conv1d(bad_c, None, x, B, KC, T, D, K, 2, out)
        with pytest.raises(AssertionError, match="cache "):
            ops.conv_cache_update(bad_c, None, x, B, KC, T, D)
    with pytest.raises(AssertionError):
        ops.conv_cache_update(None, None, x, B, KC, T, D)
    with pytest.raises(AssertionError, match="out"):
        ops.im2col_conv1d(cache, None, x, B, KC, T, D, K, 2, torch.zeros(B * 2, D * K - 1))
