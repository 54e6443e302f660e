"""The sampler model's tolerance cannot hide a wrong kernel (tests/sampler_ref.py).

The model is run against mutated copies of itself over the tables the GPU test uses
(tests/test_sampler_kernels_gpu.py).  Under the acceptance rule every mutant must be rejected: a draw mutant fails on at
least half the draws of at least one case, a set mutant differs in the kept mask on at least one case.  The two
conditions the acceptance rule rests on are asserted for every case from the model alone: the share of draws within
delta of a CDF edge is at most 5 %, and every top-p value keeps 64 delta from the cumulative masses around it.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as R  # noqa: E402


def _settings():
    for g in R.dist_groups():
        for s in g.settings:
            yield g, s


def test_u01_matches_a_second_implementation():
    """The stream in Python integers against the same recurrence in wrapping uint64 arithmetic; known precedence."""
    def ref(seed, key, step):
        with np.errstate(over="ignore"):
            u = np.uint64
            x = u(seed) ^ (u(0x9E37) * (u(key) + u(1)) + u(step))
            x = x + u(0x9E3779B97F4A7C15)
            z = (x ^ (x >> u(30))) * u(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
            z = z ^ (z >> u(31))
            return float(np.float32(np.uint32(z >> u(40))) * np.float32(1.0 / 16777216.0))
    rng = np.random.default_rng(1)
    for _ in range(200):
        seed, key, step = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 31)), int(rng.integers(0, 2 ** 31))
        assert R.u01(seed, key, step) == ref(seed, key, step)
        assert 0.0 <= R.u01(seed, key, step) < 1.0
    assert R.u01(5, 3, 7) != R.u01(5, 3, 7, mut="prec")


def test_delta_is_the_documented_formula():
    assert R.delta("general", 1000, 0) == 51 * 2.0 ** -24 + 2 * 2.0 ** -22
    assert R.delta("general", 5000, 100) == 63 * 2.0 ** -24 + 2 * 2.0 ** -22
    assert R.delta("small", 5000, 64) == 130 * 2.0 ** -24 + 2 * 2.0 ** -22
    assert R.delta("small", 5, 2) == 6 * 2.0 ** -24 + 2 * 2.0 ** -22


def test_distribution_table_conditions():
    """Every setting reaches the path it carries and keeps the top-p margin; the table covers what it claims."""
    seen = set()
    n = 0
    for g, (k, T, p, kind, path) in _settings():
        m = R.model(g.row, k, T, p, g.ban)
        assert m.path == path, (g.name, k)
        assert abs(m.prob.sum() - 1.0) < 1e-12 and m.kept.any() and not (0 <= g.ban < g.V and m.kept[g.ban])
        if kind == "exact":
            assert m.margin == 0.0 and np.all(m.e == 1.0) and (len(m.e) & (len(m.e) - 1)) == 0, g.name
        elif kind != "none":
            assert m.margin >= R.MARGIN * m.delta, (g.name, k, T, p, kind, m.margin / m.delta)
        seen.add((g.fam, path))
        seen.add((kind, path))
        seen.add((g.bank, path))
        seen.add(("V", g.V, path))
        if kind == "tie":       # does the kept set end inside a group of equal logits?
            nk = int(m.kept.sum())
            cut = nk < len(m.gkey) and m.gkey[nk - 1] == m.gkey[nk]
            seen.add(("tie", path, "first" if cut and nk == 1 else "cut" if cut else "whole"))
        n += 1
    for path in ("small", "general"):
        for fam in R.FAMS:
            assert (fam, path) in seen, (fam, path)
        for kind in ("none", "mid", "first", "tie"):
            assert (kind, path) in seen, (kind, path)
        for bk in R.BANS:
            assert (bk, path) in seen, (bk, path)
        for V in R.VS:
            assert ("V", V, path) in seen, (V, path)
    assert ("tie", "small", "cut") in seen and ("tie", "general", "whole") in seen
    assert ("tie", "general", "cut") not in seen
    assert ("exact", "small") in seen
    assert n > 1000


def test_draw_table_conditions():
    """Ambiguous draws are at most 5 % per case, the top-p margin holds, every path is there, and the model's own
    draws pass its own acceptance rule (all of them, none skipped)."""
    paths = set()
    for c in R.draw_cases():
        m = R.model(c.row, c.k, c.T, c.p, c.ban)
        assert m.path == c.path
        paths.add(m.path)
        us = R.stream_us(c.seed, c.keys, c.steps)
        got, want = R.ambiguous_share(m, us)
        print(f"{c.name}: path {m.path}, kept {int(m.kept.sum())}, delta {m.delta:.3g}, ambiguous {got:.4f} "
              f"(predicted {want:.4f})")
        assert got <= R.AMBIG_MAX and want <= R.AMBIG_MAX, c.name
        assert c.p == 0.0 or m.margin >= R.MARGIN * m.delta, c.name
        assert all(R.accepted(m, R.pick(m, u), u) for u in us), c.name
        assert len(set(c.keys.tolist())) == R.NSTREAM and sorted(c.keys.tolist()) != list(range(R.NSTREAM))
    assert paths == {"small", "general"}


@pytest.mark.parametrize("mut", R.DRAW_MUTANTS)
def test_draw_mutant_is_rejected(mut):
    worst = 0.0
    for c in R.draw_cases():
        true = R.model(c.row, c.k, c.T, c.p, c.ban)
        wrong = R.model(c.row, c.k, c.T, c.p, c.ban, mut=(mut,))
        us, um = R.stream_us(c.seed, c.keys, c.steps), R.stream_us(c.seed, c.keys, c.steps, mut=(mut,))
        ids = [R.pick(wrong, u, mut=(mut,)) for u in um]
        worst = max(worst, float(np.mean([not R.accepted(true, i, u) for i, u in zip(ids, us)])))
    assert worst >= 0.5, (mut, worst)


@pytest.mark.parametrize("mut", R.SET_MUTANTS)
def test_set_mutant_is_rejected(mut):
    for g, (k, T, p, kind, path) in _settings():
        true = R.model(g.row, k, T, p, g.ban)
        wrong = R.model(g.row, k, T, p, g.ban, mut=(mut,))
        if not np.array_equal(true.kept, wrong.kept):
            ok, err = R.probs_error(true, wrong.prob)
            assert not ok or err > 1.0
            return
    pytest.fail(f"mutant {mut} keeps the same set on every case")


def test_probability_bound_rejects_a_wrong_value():
    """A distribution off by 4 delta on one token, or with the temperature dropped, is outside the bound."""
    g = next(g for g in R.dist_groups() if g.fam == "wide" and g.V == 1000 and g.bank == "none")
    for k, T in ((5, 0.7), (0, 0.7)):
        m = R.model(g.row, k, T, 0.0, g.ban)
        assert R.probs_error(m, m.prob.astype(np.float32))[1] <= 1.0
        bad = m.prob.copy()
        i = int(np.argmax(bad))
        bad[i] *= 1 + 4 * m.delta
        assert R.probs_error(m, bad)[1] > 1.0
        path = "small" if k else "general"
        assert R.probs_error(m, R.model(g.row, k, T, 0.0, g.ban, mut=(f"no_T_{path}",)).prob)[1] > 1.0
