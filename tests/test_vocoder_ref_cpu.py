"""The vocoder kernel tests' error bound E (tests/vocoder_ref.py) cannot hide a wrong kernel: for every case of the
tables the GPU tests run, a deliberately wrong reference differs from the true one by more than E somewhere.

Mutations every case must catch wherever they change the computation at all (a 5-step case has no tile boundary,
a case without leaky ReLU nothing to skip): (a) the last tap dropped, (b) the window read one row late in the
first 16 rows after a time-tile boundary, (c) the leaky ReLU skipped, (d) bias / res2 / gadd / oscale dropped,
whichever the case uses.  Every k_conv_cl / k_conv_pair instantiation has a case with a tile boundary and one with
the leaky ReLU.  Caught in at least one case of each family: (e) x rounded to bf16 (the lo half of the hi + lo
split lost), (f) the pair step's c1 output not zeroed outside [0, T)."""
import pytest
import torch

import vocoder_ref as vr
from fo.codec import CodecEngine


def caught(ref, mutated):
    return any(bool(((ym - y).abs() > E).any()) for (y, E), (ym, _) in zip(ref, mutated))


def conv_mutations(case, ms):
    muts = ["tap"]
    if any(m.Tq > case.tw for m in ms):
        muts.append("late")
    if any(m.pre for m in ms):
        muts.append("leaky")
    m0s = ms[:1] if case.summed else ms
    muts += [n for n, used in (("bias", any(m.bias is not None for m in ms)),
                               ("res2", any(m.res2 is not None for m in ms)),
                               ("gadd", any(m.gadd is not None for m in m0s)),
                               ("oscale", any(m.oscale != 1.0 for m in m0s))) if used]
    return muts


@pytest.mark.parametrize("case", vr.CONV_CASES + vr.MULTI_CASES, ids=lambda c: c.name)
def test_conv_bound_catches_mutations(case):
    ms = case.build()
    for i, grp in enumerate([ms] if case.summed else [[m] for m in ms]):   # every output on its own
        (y, E), = vr.conv_ref(grp, case.summed)
        assert bool((E > 0).all())
        for mut in conv_mutations(case, grp):
            ym, _ = vr.conv_ref(grp, case.summed, mut=(mut,), tw=case.tw)[0]
            assert bool(((ym - y).abs() > E).any()), (i, mut)


def test_every_conv_instantiation_has_a_boundary_and_a_leaky_case():
    for inst in [s[0] for s in vr.SMALL] + ["<4,2,16>", "<4,2,32>"]:
        cases = [c for c in vr.CONV_CASES if c.inst == inst]
        muts = [conv_mutations(c, c.build()) for c in cases]
        assert any("late" in m for m in muts) and any("leaky" in m for m in muts), inst
        for opt in ("bias", "res2", "gadd", "oscale"):
            assert any(opt in m for m in muts), (inst, opt)
        # the (11, 5) boundary case: a 50-row halo across the tile boundary
        assert any(m.K == 11 and m.dil == 5 and m.Tq > c.tw for c in cases for m in c.build()), inst


def test_conv_bound_catches_lost_lo_half():
    hits = [c.name for c in vr.CONV_CASES if c.api == "cl"
            and caught(vr.conv_ref(c.build()), vr.conv_ref(c.build(), mut=("bf16",)))]
    assert hits, "no conv_cl case tells a bf16-rounded input from the hi + lo split"


@pytest.mark.parametrize("case", vr.PAIR_CASES, ids=lambda c: c.name)
def test_pair_bound_catches_mutations(case):
    ms, gadd = case.build()
    kw = dict(summed=case.summed, oscale=case.oscale, gadd=gadd)
    muts = ["tap", "leaky", "bias"] + (["late"] if case.T > case.tw else [])
    muts += ["gadd", "oscale"] if case.summed else []
    for i, grp in enumerate([ms] if case.summed else [[m] for m in ms]):   # every output on its own
        (y, E), = vr.pair_ref(grp, case.T, **kw)
        assert bool((E > 0).all())
        for mut in muts:
            ym, _ = vr.pair_ref(grp, case.T, mut=(mut,), tw=case.tw, **kw)[0]
            assert bool(((ym - y).abs() > E).any()), (i, mut)


@pytest.mark.parametrize("mut", ["bf16", "nozero"])
def test_pair_bound_catches_in_some_case(mut):
    hits = {}
    for c in vr.PAIR_CASES:
        ms, gadd = c.build()
        kw = dict(summed=c.summed, oscale=c.oscale, gadd=gadd)
        hits[c.name] = caught(vr.pair_ref(ms, c.T, **kw), vr.pair_ref(ms, c.T, mut=(mut,), **kw))
    for C in (16, 32, 64):   # in every instantiation
        assert any(v for k, v in hits.items() if f"/C{C}/" in k), (mut, C)
    if mut == "nozero":      # c2 reads past the ends in every case
        assert all(hits.values()), [k for k, v in hits.items() if not v]


@pytest.mark.parametrize("u,k", vr.POLY_UK)
def test_polyphase_members_equal_conv_transpose_and_catch_mutations(u, k):
    """CodecEngine.polyphase's (j0, pad) bookkeeping turns ConvTranspose1d into u plain convolutions exactly,
    odd k - u included, and the per-phase bound catches the mutations."""
    phases = CodecEngine.polyphase(u, k)
    assert [p[0] for p in phases] == list(range(u))
    lost = False
    for Cin in (32, 128):
        for Tin in (1, 7, 70):
            x, W, b, ms = vr.poly_case(u, k, Cin, Tin, phases)
            want = vr.convT_ref(x, W, b, u, k)
            ref = vr.conv_ref(ms)
            full = vr.interleave(ms, [y for y, _ in ref])
            assert full.shape == want.shape and want.shape[1] == (Tin - 1) * u - 2 * ((k - u) // 2) + k
            assert torch.allclose(full, want, rtol=0, atol=1e-12)   # every position written, same numbers
            for mut in ("leaky", "bias") + (("tap",) if Tin > 1 else ()):
                assert caught(ref, vr.conv_ref(ms, mut=(mut,))), (Cin, Tin, mut)
            if Tin == 70:   # one phase's taps swapped for its neighbour's: a wrong tap in one component
                wrong = vr.poly_members(x, W, b, u, k, [phases[0][:1] + phases[1][1:2] + phases[0][2:]] + phases[1:])
                if wrong[0].K == ms[0].K:
                    assert caught(ref, vr.conv_ref(wrong)), (Cin, "j0")
            lost |= caught(ref, vr.conv_ref(ms, mut=("bf16",)))
    assert lost, "no polyphase case tells a bf16-rounded input from the hi + lo split"
