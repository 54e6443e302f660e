"""csrc/fo_sample.hip against the float64 model of tests/sampler_ref.py: distributions, draws, the split arg-max,
the fused next-input step and the repetition penalty.  Every output buffer is surrounded by sentinel values that must
come back bit-identical, and the SampleCheck word must be clear after every launch of a well-formed row.

Each test prints its figures (max error / delta, ambiguous draws observed against predicted) before it asserts.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_F = 12345.678
SENT_I = -777
PAD = 1e30      # logits padding: larger than any logit, so a read past V (or before the view) wins the arg-max


@pytest.fixture(scope="module")
def chk(dev):
    from fo import ops
    c = ops.SampleCheck()
    yield c
    c.free()


def flag(chk):
    torch.cuda.synchronize()
    v = int(chk.buf.np[0, 0])
    chk.buf.np[0, 0] = 0
    return v


def guarded(shape, dtype, dev):
    """A buffer of shape + one guard row before and after (and guard columns as given by the caller's view)."""
    sent = SENT_F if dtype == torch.float32 else SENT_I
    return torch.full(shape, sent, dtype=dtype, device=dev)


def assert_guard(buf, inner, what):
    """Everything of buf outside the boolean mask `inner` still holds the sentinel."""
    sent = SENT_F if buf.dtype == torch.float32 else SENT_I
    want = torch.full_like(buf, sent)
    assert torch.equal(torch.where(inner, want, buf), want), f"{what}: a guard value was overwritten"


def i32(a, dev):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)


def f32(a, dev):
    return torch.as_tensor(np.asarray(a, np.float32)).to(dev)


def shared(row, B, dev):
    """B rows that are one row (ld == 0)"""
    t = torch.from_numpy(np.array(row)).to(dev)
    lg = t.as_strided((B, t.numel()), (0, 1))
    assert lg.stride(0) == 0
    return lg


# ------------------------------------------------------------------------------------------------ distributions
def run_group(ops, dev, chk, g):
    """One launch of fo_sample_probs over the group's settings; returns the [B, V] distributions."""
    B, V = len(g.settings), g.V
    pb = guarded((B + 2, V + 5), torch.float32, dev)
    ib = guarded((B + 2,), torch.int32, dev)
    ops.sample_probs(shared(g.row, B, dev), V, ib[1:B + 1], pb[1:B + 1], i32([s[0] for s in g.settings], dev),
                     f32([s[1] for s in g.settings], dev), f32([s[2] for s in g.settings], dev), seed=11,
                     step=i32(np.arange(B), dev), B=B, ban_id=g.ban, err=chk)
    assert flag(chk) == 0, g.name
    inner = torch.zeros_like(pb, dtype=torch.bool)
    inner[1:B + 1, :V] = True
    assert_guard(pb, inner, g.name + " probs")
    ii = torch.zeros_like(ib, dtype=torch.bool)
    ii[1:B + 1] = True
    assert_guard(ib, ii, g.name + " ids")
    return pb[1:B + 1, :V].cpu().numpy(), ib[1:B + 1].cpu().numpy()


@pytest.mark.parametrize("V", R.VS)
def test_distributions(dev, chk, V):
    """fo_sample_probs over the table at one V: support exact, values within delta (floor 2^-32), the drawn id kept."""
    from fo import ops
    worst = {"small": 0.0, "general": 0.0}
    n = 0
    for g in R.dist_groups():
        if g.V != V or g.fam in ("fin64", "dyadic"):
            continue
        got, ids = run_group(ops, dev, chk, g)
        for r, (k, T, p, kind, path) in enumerate(g.settings):
            m = R.model(g.row, k, T, p, g.ban)
            ok, err = R.probs_error(m, got[r])
            worst[path] = max(worst[path], err)
            assert ok, f"{g.name} k={k} T={T} p={p} ({kind}): support differs " \
                       f"(kernel {np.flatnonzero(got[r] > 0)[:12]}, model {np.flatnonzero(m.kept)[:12]})"
            assert err <= 1.0, f"{g.name} k={k} T={T} p={p} ({kind}): error {err:.3f} delta"
            assert m.kept[ids[r]], (g.name, k, ids[r])
            n += 1
    print(f"V={V}: {n} settings, max error / delta: small {worst['small']:.3f}, general {worst['general']:.3f}")


def test_distributions_k64_against_k65_and_exact_boundary(dev, chk):
    """On a tie-free row with 64 finite logits k = 64 (small path) and k = 65 (general path) keep the same support
    and agree within 2 delta; a top-p value exactly on a cumulative mass keeps the token it reaches (<=)."""
    from fo import ops
    for g in R.dist_groups():
        if g.fam not in ("fin64", "dyadic"):
            continue
        got, _ = run_group(ops, dev, chk, g)
        by = {}
        for r, (k, T, p, kind, path) in enumerate(g.settings):
            m = R.model(g.row, k, T, p, g.ban)
            ok, err = R.probs_error(m, got[r])
            assert ok and err <= 1.0, (g.name, k, T, p, kind, err)
            by.setdefault((T, p), {})[k] = (got[r].astype(np.float64), m.delta)
        if g.fam == "dyadic":
            assert int((got[0] > 0).sum()) == 2 and np.all(got[0][got[0] > 0] == 0.5)
            continue
        for (T, p), d in by.items():
            (a, da), (b, db) = d[64], d[65]
            assert np.array_equal(a > 0, b > 0), (g.name, T, p)
            assert np.all(np.abs(a - b) <= 2 * max(da, db) * np.maximum(a, b) + R.FLOOR), (g.name, T, p)


# ------------------------------------------------------------------------------------------------ draws
def run_draws(ops, dev, chk, c, rows=None):
    rows = np.arange(R.NSTREAM) if rows is None else np.asarray(rows)
    B = len(rows)
    ib = guarded((B + 2,), torch.int32, dev)
    mb = guarded((B + 2,), torch.float32, dev)
    ops.sample(shared(c.row, B, dev), c.V, ib[1:B + 1], i32(np.full(B, c.k), dev), f32(np.full(B, c.T), dev),
               f32(np.full(B, c.p), dev), seed=c.seed, step=i32(c.steps[rows], dev), out_max=mb[1:B + 1], B=B,
               ban_id=c.ban, key=i32(c.keys[rows], dev), err=chk)
    assert flag(chk) == 0, c.name
    ids, mx = ib.cpu().numpy(), mb.cpu().numpy()
    assert ids[0] == SENT_I and ids[-1] == SENT_I and mx[0] == np.float32(SENT_F) and mx[-1] == np.float32(SENT_F)
    return ids[1:-1], mx[1:-1]


@pytest.mark.parametrize("name", [c.name for c in R.draw_cases()])
def test_draws(dev, chk, name):
    """512 streams of one row: every id lies in the CDF interval its u selects (+- delta), none skipped."""
    from fo import ops
    c = next(c for c in R.draw_cases() if c.name == name)
    m = R.model(c.row, c.k, c.T, c.p, c.ban)
    us = R.stream_us(c.seed, c.keys, c.steps)
    ids, mx = run_draws(ops, dev, chk, c)
    ex = np.array([R.excess(m, int(i), u) for i, u in zip(ids, us)])
    amb, pred = R.ambiguous_share(m, us)
    differ = float(np.mean([int(i) != R.pick(m, u) for i, u in zip(ids, us)]))
    print(f"{name}: path {m.path}, kept {int(m.kept.sum())}, max excess / delta {ex.max():.3f}, ambiguous draws "
          f"{amb:.4f} (predicted {pred:.4f}), ids off the float64 pick {differ:.4f}")
    assert amb <= R.AMBIG_MAX
    bad = np.flatnonzero(ex > 1.0)
    assert not len(bad), f"{name}: {len(bad)} of {len(ids)} draws rejected, first: stream {bad[0]} id {ids[bad[0]]} " \
                         f"u {us[bad[0]]!r} want {R.pick(m, us[bad[0]])} excess {ex[bad[0]]}"
    allowed = np.array(c.row)
    if 0 <= c.ban < c.V:
        allowed[c.ban] = -np.inf
    assert np.all(mx == allowed.max())


def test_draws_follow_the_key_not_the_row(dev, chk):
    """Five of the streams as a batch of their own (same keys and steps) draw what they drew in the full batch."""
    from fo import ops
    c = next(c for c in R.draw_cases() if c.name == "flat-1025")
    full, _ = run_draws(ops, dev, chk, c)
    rows = [3, 77, 200, 301, 511]
    part, _ = run_draws(ops, dev, chk, c, rows)
    assert len(set(full[rows].tolist())) > 1
    assert np.array_equal(part, full[rows])


def test_draws_mixed_paths_one_launch(dev, chk):
    """Rows with k = 1, 5, 0 and 200 in one grid, each its own row of a padded buffer (ld = V + 3)."""
    from fo import ops
    V, B = 4096, 8
    fams = ("wide", "narrow", "quant", "inf40")
    ks = [1, 5, 0, 200, 200, 0, 5, 1]
    Ts = [1.0, 0.7, 1.6, 1.0, 0.25, 0.7, 1.6, 1.0]
    seed, keys, steps = R.streams("mixed", B)
    buf = torch.full((B, V + 3), PAD, dtype=torch.float32, device=dev)
    rows = [R.make_row(fams[r % 4], V) for r in range(B)]
    buf[:, :V] = torch.from_numpy(np.stack(rows)).to(dev)
    ib = guarded((B + 2,), torch.int32, dev)
    mb = guarded((B + 2,), torch.float32, dev)
    ban = 17
    ops.sample(buf, V, ib[1:B + 1], i32(ks, dev), f32(Ts, dev), f32(np.zeros(B), dev), seed=seed, step=i32(steps, dev),
               out_max=mb[1:B + 1], B=B, ban_id=ban, key=i32(keys, dev), err=chk)
    assert flag(chk) == 0
    ids, mx = ib.cpu().numpy(), mb.cpu().numpy()
    assert ids[0] == SENT_I and ids[-1] == SENT_I and mx[0] == np.float32(SENT_F) and mx[-1] == np.float32(SENT_F)
    us = R.stream_us(seed, keys, steps)
    paths = set()
    for r in range(B):
        m = R.model(rows[r], ks[r], Ts[r], 0.0, ban)
        paths.add((ks[r], m.path))
        assert R.accepted(m, int(ids[1 + r]), us[r]), (r, ks[r], ids[1 + r], R.pick(m, us[r]))
        a = np.array(rows[r])
        a[ban] = -np.inf
        assert mx[1 + r] == a.max()
    assert paths == {(1, "small"), (5, "small"), (0, "general"), (200, "general")}


def test_degenerate_rows_set_the_check_word(dev, chk):
    """A row of -inf only sets the SampleCheck word on every path; the id stays inside the table."""
    from fo import ops
    V = 100
    row = np.full(V, -np.inf, np.float32)
    for k in (1, 5, 0, 70):
        ib = guarded((3,), torch.int32, dev)
        ops.sample(shared(row, 1, dev), V, ib[1:2], i32([k], dev), f32([1.0], dev), f32([0.0], dev), seed=1, B=1,
                   err=chk)
        assert flag(chk) == 1, k
        ids = ib.cpu().numpy()
        assert ids[0] == SENT_I and ids[2] == SENT_I and 0 <= ids[1] < V


# ------------------------------------------------------------------------------------------------ arg-max
def argmax_rows(V):
    """Three rows: the maximum in the last element (last chunk, ragged tail), tied across two chunks (smaller index
    wins), and inside a full 8-wide group of the third chunk; second maxima elsewhere for the banned launches."""
    rng = R.rng_of(f"argmax/{V}")
    a = rng.standard_normal((3, V)).astype(np.float32)
    a[0, V - 1], a[0, 1234] = 50.0, 49.0
    a[1, 2048 + 5], a[1, 100], a[1, 4100] = 51.0, 51.0, 51.0
    a[2, 4099], a[2, V - 3] = 60.0, 59.0
    return a


@pytest.mark.parametrize("V", [8191, 8192, 8200, 10007])
def test_argmax_split_and_single(dev, chk, V):
    """k = 1 with and without the split arg-max workspace, at row strides V, V + 3 and V + 4 (vector and scalar
    loads), the ban inside a full group and inside the ragged tail, and a view offset by one column (row stride a
    multiple of 4, base pointer not 16-byte aligned)."""
    from fo import ops
    a = argmax_rows(V)
    B = 3
    lds = [(V, 0), (V + 3, 0), (V + 4, 0), ((V + 8) // 4 * 4, 1)]
    for ld, off in lds:
        buf = torch.full((B, ld), PAD, dtype=torch.float32, device=dev)
        buf[:, off:off + V] = torch.from_numpy(a).to(dev)
        lg = buf[:, off:off + V]
        assert lg.stride(0) == ld and (off == 0 or (ld % 4 == 0 and lg.data_ptr() % 16 == 4))
        for ban in (-1, 4099, V - 1, V + 2):
            want = a.copy()
            if 0 <= ban < V:
                want[:, ban] = -np.inf
            res = {}
            for ws in (False, True):
                ib = guarded((B + 2,), torch.int32, dev)
                mb = guarded((B + 2,), torch.float32, dev)
                ops.sample(lg, V, ib[1:B + 1], out_max=mb[1:B + 1], B=B, ban_id=ban, err=chk, argmax_ws=ws)
                assert flag(chk) == 0
                ids, mx = ib.cpu().numpy(), mb.cpu().numpy()
                assert ids[0] == SENT_I and ids[-1] == SENT_I
                assert mx[0] == np.float32(SENT_F) and mx[-1] == np.float32(SENT_F)
                assert ids[1:-1].tolist() == want.argmax(1).tolist(), (V, ld, off, ban, ws)   # first index of the max
                assert np.array_equal(mx[1:-1], want.max(1)), (V, ld, off, ban, ws)
                res[ws] = ids
            assert np.array_equal(res[False], res[True])
        assert torch.equal(buf[:, off:off + V].cpu(), torch.from_numpy(a))


# ------------------------------------------------------------------------------------------------ next input
def embed_setup(dev, D, V=300, B=5):
    g = torch.Generator().manual_seed(D)
    table = torch.randn(V, D + 8, generator=g).bfloat16().to(dev)
    gamma = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dev)
    rows = np.stack([R.make_row(("wide", "narrow", "quant", "inf40", "zeros")[r], 1000)[:V] for r in range(B)])
    ks, Ts = [1, 5, 0, 100, 2], [1.0, 0.7, 1.6, 1.0, 0.25]
    return table, gamma, rows, ks, Ts


def check_next_input(ops, dev, ids, table, gamma, D, xb, hb, B, eps):
    idt = i32(ids, dev)
    emb = table[:, :D]
    assert torch.equal(xb[1:B + 1, :D], emb[idt.long()].float()), "x is not the table row"
    xg = ops.gather_rows(emb, idt, D=D)
    href = ops.rmsnorm(xg, gamma, eps)
    assert torch.equal(xg, xb[1:B + 1, :D].contiguous())
    assert torch.equal(hb[1:B + 1, :D].contiguous(), href), "h differs from gather_rows + rmsnorm"
    inner = torch.zeros_like(xb, dtype=torch.bool)
    inner[1:B + 1, :D] = True
    assert_guard(xb, inner, "x")
    assert_guard(hb, inner, "h")


@pytest.mark.parametrize("D", [4, 896, 1024, 4096])
def test_sample_embed_next_input(dev, chk, D):
    """fo_sample_embed: ids as fo_sample draws them, x the bf16 table row exactly, h bit-identical to gather_rows +
    rmsnorm, the history row written through hist_row, nothing else touched (emb_ld, ldx, ldh above D)."""
    from fo import ops
    B, V, eps, ban = 5, 300, 1e-6, 7
    table, gamma, rows, ks, Ts = embed_setup(dev, D)
    seed, keys, steps = R.streams(f"embed/{D}", B)
    lg = torch.from_numpy(rows).to(dev)
    kw = dict(top_k=i32(ks, dev), temperature=f32(Ts, dev), top_p=f32(np.zeros(B), dev), seed=seed,
              step=i32(steps, dev), B=B, ban_id=ban, key=i32(keys, dev), err=chk)
    want = ops.sample(lg, V, torch.empty(B, dtype=torch.int32, device=dev), **kw).cpu().numpy()
    assert flag(chk) == 0
    us = R.stream_us(seed, keys, steps)
    for r in range(B):
        assert R.accepted(R.model(rows[r], ks[r], Ts[r], 0.0, ban), int(want[r]), us[r]), r
    xb = guarded((B + 2, D + 4), torch.float32, dev)
    hb = guarded((B + 2, D + 4), torch.float32, dev)
    ib = guarded((B + 2,), torch.int32, dev)
    hist_ld, hrow = B + 3, 2
    hist = guarded((4, hist_ld), torch.int32, dev)
    ops.sample_embed(lg, V, ib[1:B + 1], table[:, :D], xb[1:B + 1, :D], gamma, eps, hb[1:B + 1, :D],
                     hist_ptr=hist.data_ptr(), hist_row=i32([hrow], dev), hist_ld=hist_ld, **kw)
    assert flag(chk) == 0
    ids = ib.cpu().numpy()
    assert ids[0] == SENT_I and ids[-1] == SENT_I and np.array_equal(ids[1:-1], want)
    check_next_input(ops, dev, want, table, gamma, D, xb, hb, B, eps)
    inner = torch.zeros_like(hist, dtype=torch.bool)
    inner[hrow, :B] = True
    assert_guard(hist, inner, "hist")
    assert np.array_equal(hist[hrow, :B].cpu().numpy(), want)


@pytest.mark.parametrize("D", [4, 896, 1024, 4096])
def test_sample_embed_advances_the_decode_metadata(dev, chk, D):
    """With the metadata block every field moves to its next value on the device: position, visible keys and step
    + 1, the slot from the block table (page crossing at L % PS == PS - 1 and == 0; L / PS == maxb gives page 0),
    the counter word once, the history row = the row's own step; the block table stays as it was."""
    from fo import ops
    B, V, eps, ban, PS, maxb = 5, 300, 1e-6, 7, 4, 3
    table, gamma, rows, ks, Ts = embed_setup(dev, D)
    seed, keys, _ = R.streams(f"embed-meta/{D}", B)
    L = np.array([3, 4, 12, 5, 0])            # PS - 1, 0 mod PS, maxb * PS (past the table), mid-page, empty
    pos = np.array([103, 204, 312, 405, 500])
    steps = np.array([4, 0, 2, 1, 3])
    bt = np.array([[9, 2, 5], [1, 8, 3], [4, 6, 7], [11, 10, 12], [13, 14, 15]])
    slot0 = np.array([77, 78, 79, 80, 81])
    n = 5 * B + 1 + B * maxb
    old = np.concatenate([pos, slot0, L, steps, keys, [40], bt.ravel()]).astype(np.int32)
    assert old.size == n
    mb = guarded((n + 2,), torch.int32, dev)
    mb[1:n + 1] = i32(old, dev)
    meta = mb[1:n + 1]
    lg = torch.from_numpy(rows).to(dev)
    kw = dict(top_k=i32(ks, dev), temperature=f32(Ts, dev), top_p=f32(np.zeros(B), dev), seed=seed, B=B, ban_id=ban,
              err=chk)
    want = ops.sample(lg, V, torch.empty(B, dtype=torch.int32, device=dev), step=i32(steps, dev), key=i32(keys, dev),
                      **kw).cpu().numpy()
    xb = guarded((B + 2, D + 4), torch.float32, dev)
    hb = guarded((B + 2, D + 4), torch.float32, dev)
    ib = guarded((B + 2,), torch.int32, dev)
    hist_ld = B + 3
    hist = guarded((6, hist_ld), torch.int32, dev)
    ops.sample_embed(lg, V, ib[1:B + 1], table[:, :D], xb[1:B + 1, :D], gamma, eps, hb[1:B + 1, :D],
                     step=meta[3 * B:4 * B], key=meta[4 * B:5 * B], hist_ptr=hist.data_ptr(), hist_ld=hist_ld, meta=meta,
                     maxb=maxb, PS=PS, **kw)
    assert flag(chk) == 0
    ids = ib.cpu().numpy()
    assert ids[0] == SENT_I and ids[-1] == SENT_I and np.array_equal(ids[1:-1], want)
    check_next_input(ops, dev, want, table, gamma, D, xb, hb, B, eps)
    pg = L // PS
    slot = np.array([(bt[r, pg[r]] if pg[r] < maxb else 0) * PS + L[r] % PS for r in range(B)])
    new = np.concatenate([pos + 1, slot, L + 1, steps + 1, keys, [41], bt.ravel()]).astype(np.int32)
    got = mb.cpu().numpy()
    assert got[0] == SENT_I and got[-1] == SENT_I
    assert np.array_equal(got[1:-1], new), (got[1:-1], new)
    inner = torch.zeros_like(hist, dtype=torch.bool)
    h = hist.cpu().numpy()
    for r in range(B):
        inner[int(steps[r]), r] = True
        assert h[steps[r], r] == want[r]
    assert_guard(hist, inner, "hist")


# ------------------------------------------------------------------------------------------------ penalty
def test_penalty_three_blocks_window_order(dev):
    """fo_penalty at B = 130 (three 64-lane blocks, rows past B untouched), ld > V, steps 0, W - 1, W and 3 W + 1
    in one launch, against a numpy loop that divides in window order, once per occurrence."""
    from fo import ops
    B, V, W, ld, pen = 130, 50, 4, 56, np.float32(1.25)
    rng = R.rng_of("penalty")
    lg = rng.standard_normal((B + 2, ld)).astype(np.float32) * 3
    win = rng.integers(-1, 6, (B + 2, W)).astype(np.int32)        # few values: duplicates in most windows; -1 ignored
    win[5] = [V, V + 3, 7, 7]                                      # ids >= V (inside the row's padding) ignored
    ids = rng.integers(0, 6, B + 2).astype(np.int32)
    ids[9], ids[10] = -1, V + 2
    step = np.array([(0, W - 1, W, 3 * W + 1)[r % 4] for r in range(B + 2)], np.int32)
    want_lg, want_win = lg.copy(), win.copy()
    for r in range(B):
        st = int(step[r])
        want_win[r, st % W] = ids[r]
        for j in range(min(st + 1, W)):
            t = int(want_win[r, j])
            if 0 <= t < V:
                want_lg[r, t] = np.float32(want_lg[r, t] / pen)
    tl, tw = torch.from_numpy(lg).to(dev), torch.from_numpy(win).to(dev)
    ops.penalty(tl, V, i32(ids, dev), tw, i32(step, dev), float(pen), B=B)
    torch.cuda.synchronize()
    assert np.array_equal(tw.cpu().numpy(), want_win)
    assert np.array_equal(tl.cpu().numpy(), want_lg)
    assert np.array_equal(want_lg[B:], lg[B:]) and not np.array_equal(want_lg[:B], lg[:B])
