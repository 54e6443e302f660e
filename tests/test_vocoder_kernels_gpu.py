"""The vocoder's MFMA conv kernels (csrc/fo_vocoder.hip), launched through fo.ops one at a time, against the
float64 reference of tests/vocoder_ref.py: every output element within the derived bound E, guard rows and
positions a launch may not write bit-identical.  The table of cases and the instantiation each one reaches by
conv_launch's rules is next to the cases, in vocoder_ref.py; tests/test_vocoder_ref_cpu.py shows that E cannot
hide a wrong kernel.

Observed max(err / E) on an MI355X: conv_cl 0.242, conv_cl_multi 0.200, polyphase 0.148, pair 0.038,
conv_post 0.003 (the same conv_cl and pair figures under FO_CONV_CK=64 / 16, FO_CONV_HALFT=1, FO_CONV_PREFETCH=1:
the greatest ratios belong to 16-channel cases, whose bound is smallest and whose chunking no switch changes).
"""
import os
import subprocess
import sys

import pytest
import torch

import vocoder_ref as vr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from fo import ops
    yield ops
    print("\nobserved max(err / E):", {k: round(v, 4) for k, v in vr.OBSERVED.items()})


# ---------------------------------------------------------------------------------------- k_conv_cl, k_conv_pair
@pytest.mark.parametrize("case", vr.CONV_CASES + vr.MULTI_CASES, ids=lambda c: c.name)
def test_conv_cl_matches_float64(ops, dev, case):
    r = vr.run_conv_case(case, dev)
    print(f"{case.name}: max err/E {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("case", vr.PAIR_CASES, ids=lambda c: c.name)
def test_conv_pair_matches_float64(ops, dev, case):
    r = vr.run_pair_case(case, dev)
    print(f"{case.name}: max err/E {r:.4f}")
    assert r <= 1.0


# ---------------------------------------------------------------------------------------- polyphase ConvTranspose1d
@pytest.mark.parametrize("u,k", vr.POLY_UK)
@pytest.mark.parametrize("Cin", [32, 128])
def test_polyphase_conv_transpose_matches_float64(ops, dev, u, k, Cin):
    """leaky -> ConvTranspose1d(Cin -> Cin / 2, stride u) as CodecEngine launches it (its polyphase() bookkeeping,
    PackedConv(transposed=...)): one conv_cl_multi, and u conv_cl calls, against float64 conv_transpose1d, the
    output length included.  (2,5) and (3,8) have odd k - u.  Cin 32 -> k_conv_cl<1,8,32>, 128 -> <2,2,32>."""
    from fo.codec import CodecEngine
    phases = CodecEngine.polyphase(u, k)
    worst = 0.0
    for Tin in (1, 7, 70):
        x, W, b, ms = vr.poly_case(u, k, Cin, Tin, phases)
        want = vr.convT_ref(x, W, b, u, k)
        assert want.shape[1] == ms[0].Tout and sum(m.Tq for m in ms) == want.shape[1]
        E = vr.interleave(ms, [e for _, e in vr.conv_ref(ms)])
        Wd, bd = W.to(dev).bfloat16(), b.to(dev)
        pcs = [ops.PackedConv(Wd, bd, transposed=(j0, u)) for _, j0, _ in phases]
        assert [pc.K for pc in pcs] == [m.K for m in ms]
        out = vr.launch_conv(ops, ms, 2, Cin, Cin // 2, dev, "multi", False, pcs=pcs)["up"]
        assert bool(out.mask.all())   # the phases cover every output step
        worst = max(worst, vr.ratio(out.check(f"{u},{k},{Tin},multi"), want, E))
        # one conv_cl per phase, each into a sentinel-filled output of its own: the other phases' steps stay untouched
        own = [vr.NS(**{**vars(m), "out_key": None}) for m in ms]
        outs = vr.launch_conv(ops, own, 2, Cin, Cin // 2, dev, "cl", False, pcs=pcs)
        for i, m in enumerate(ms):
            got = outs[i].check(f"{u},{k},{Tin},cl,{i}")
            worst = max(worst, vr.ratio(got[:, vr.pos(m)], want[:, vr.pos(m)], E[:, vr.pos(m)]))
    print(f"polyphase u={u} k={k} Cin={Cin}: max err/E {vr.note('polyphase', worst):.4f}")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------- small kernels
def test_codec_embed_cl_rows_and_out_of_range_ids(ops, dev):
    n_codes, E, B, T = 60, 512, 2, 9
    g = vr.gen("embed")
    table = vr.acts(g, n_codes + 1, E).bfloat16()   # one row past n_codes: must never be read as an embedding
    ids = torch.randint(0, n_codes, (B, T), generator=g, dtype=torch.int32)
    ids[0, 3], ids[1, 0], ids[1, 8] = n_codes, -1, n_codes - 1
    out = vr.Guarded(B, T, E, dev)
    out.mask[:] = True
    out.arm()
    ops.codec_embed_cl(table.to(dev), E, n_codes, ids.to(dev), B, T, out.t)
    torch.cuda.synchronize(dev)
    want = table.float()[ids.clamp(0, n_codes).long()]
    want[0, 3] = 0
    want[1, 0] = 0
    assert torch.equal(out.check("embed"), want)


@pytest.mark.parametrize("with_g", [False, True])
def test_scale_add_cl_matches_float64(ops, dev, with_g):
    B, T, C = 3, 37, 48
    g = vr.gen("scale_add")
    y, ga = vr.acts(g, B, T, C), (vr.acts(g, B, C) if with_g else None)
    buf = vr.Guarded(B, T, C, dev)
    buf.t.copy_(y)
    buf.mask[:] = True
    buf.arm()
    ops.scale_add_cl(buf.t, B, T, C, vr.THIRD, None if ga is None else ga.to(dev))
    torch.cuda.synchronize(dev)
    want = y.double() * vr.THIRD + (0 if ga is None else ga.double()[:, None])
    A = y.double().abs() * vr.THIRD + (0 if ga is None else ga.double().abs()[:, None])
    assert vr.ratio(buf.check("scale_add"), want, 2.0 ** -23 * A) <= 1.0   # two fp32 roundings


@pytest.mark.parametrize("C", [16, 32])
@pytest.mark.parametrize("T", [3, 300])
def test_conv_post_cl_matches_float64(ops, dev, C, T):
    B, K = 2, 7
    g = vr.gen(f"post/{C}/{T}")
    x, w, b = vr.acts(g, B, T, C), vr.weights(g, (1, C, K), K * C), vr.acts(g, 1)
    want, E = vr.post_ref(x, w, b, K, 3)
    out = vr.Guarded(B, T, 1, dev)
    out.mask[:] = True
    out.arm()
    ops.conv_post_cl(x.to(dev), B, T, C, w.to(dev).bfloat16(), b.to(dev), K, 3, vr.SLOPE, out.t)
    torch.cuda.synchronize(dev)
    r = vr.note("conv_post", vr.ratio(out.check("post")[..., 0], want, E))
    print(f"conv_post C={C} T={T}: max err/E {r:.4f}")
    assert r <= 1.0


# ---------------------------------------------------------------------------------------- refusals
def _refused(dev, launch, *bufs):
    """launch() raises RuntimeError (an error code of the entry point, no kernel runs); bufs come back untouched."""
    before = [b.clone() for b in bufs]
    with pytest.raises(RuntimeError):
        launch()
    torch.cuda.synchronize(dev)
    for b, a in zip(bufs, before):
        assert torch.equal(b.view(torch.int32), a.view(torch.int32))


def _pc(ops, dev, Cout, Cin, K, name="refuse"):
    g = vr.gen(f"{name}/{Cout}/{Cin}/{K}")
    return ops.PackedConv(vr.weights(g, (Cout, Cin, K), K * Cin).to(dev).bfloat16(), vr.acts(g, Cout).to(dev))


def test_conv_cl_refusals_leave_out_untouched(ops, dev):
    B, T, C = 2, 40, 32
    g = vr.gen("refusals")
    x, x2 = vr.acts(g, B, T, C).to(dev), vr.acts(g, B, T, C).to(dev)
    out, out2 = torch.full((B, T, C), vr.SENT, device=dev), torch.full((B, T, C), vr.SENT, device=dev)
    p3 = _pc(ops, dev, C, C, 3)
    _refused(dev, lambda: ops.conv_cl(x, B, C, T, p3, 1, 1, x), x)                       # out aliases x
    _refused(dev, lambda: ops.conv_cl_multi([ops.conv_desc(x, T, p3, 1, 1, out), ops.conv_desc(out, T, p3, 1, 1, out2)],
                                            B, C, C, dev), out, out2)                    # a member reads another's out
    _refused(dev, lambda: ops.conv_cl(x, B, C, T, _pc(ops, dev, C, C, 13), 1, 6, out), out)     # K = 13
    _refused(dev, lambda: ops.conv_cl(x, B, C, T, _pc(ops, dev, C, C, 11), 6, 30, out), out)    # dil * (K-1) = 60 > 56
    out48 = torch.full((B, T, 48), vr.SENT, device=dev)
    _refused(dev, lambda: ops.conv_cl(x, B, C, T, _pc(ops, dev, 48, C, 3), 1, 1, out48), out48)  # Cout = 48
    _refused(dev, lambda: ops.conv_cl_multi([ops.conv_desc(x, T, p3, 1, 1, out, Tq=T, Tout_total=T),
                                             ops.conv_desc(x2, T, p3, 1, 1, out, Tq=T - 1, Tout_total=T)],
                                            B, C, C, dev, summed=True), out)             # summed, different Tq


def test_conv_pair_refusals_leave_out_untouched(ops, dev):
    B, T = 2, 40
    g = vr.gen("pair refusals")
    x48, out48 = vr.acts(g, B, T, 48).to(dev), torch.full((B, T, 48), vr.SENT, device=dev)
    p3 = _pc(ops, dev, 16, 16, 3)   # (48 channels cannot even be packed: the entry refuses before it reads a weight)
    with pytest.raises(RuntimeError):
        _pc(ops, dev, 48, 48, 3)
    _refused(dev, lambda: ops.conv_pair_multi([(x48, p3, p3, 3, 1, out48)], B, 48, T, dev), out48)     # C = 48
    x, out = vr.acts(g, B, T, 16).to(dev), torch.full((B, T, 16), vr.SENT, device=dev)
    p4 = _pc(ops, dev, 16, 16, 4)
    _refused(dev, lambda: ops.conv_pair_multi([(x, p4, p4, 4, 1, out)], B, 16, T, dev), out)           # even K
    _refused(dev, lambda: ops.conv_pair_multi([(x, p3, p3, 3, 1, x)], B, 16, T, dev), x)               # out aliases x


# ---------------------------------------------------------------------------------------- engine level
@pytest.mark.parametrize("mode", ["default", "pair=False", "grouped=False"])
def test_small_grouped_engine_matches_oracle(ops, dev, mode):
    """CodecEngine at a geometry small enough for the oracle that still takes the default grouped path (rates
    2/2/2/2; stages of 128, 64, 32 and 16 channels: gadd, summed conv_cl_multi, the pair kernel), per-row global
    style tokens, against oracle.nets.Codec at test_codec_matches_golden's tolerance."""
    vr.engine_check(dev, modes=(mode,))


# ---------------------------------------------------------------------------------------- process-level A/B switches
@pytest.mark.parametrize("var,val", [("FO_CONV_CK", "64"), ("FO_CONV_CK", "16"), ("FO_CONV_HALFT", "1"),
                                     ("FO_CONV_PREFETCH", "1")])
def test_switch_in_fresh_process(dev, var, val):
    """The FO_CONV_* switches are read once per process: one fresh interpreter per setting runs the conv_cl and
    pair tables and the small engine (vocoder_ref.main), and exits non-zero on a mismatch.  Under a non-default
    FO_CONV_CK the pair cases fo_conv_pair_multi documents as refused must raise."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("FO_CONV_")}
    env[var] = val
    r = subprocess.run([sys.executable, os.path.abspath(vr.__file__)], env=env, capture_output=True, text=True,
                       timeout=240)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, f"{var}={val}: exit {r.returncode}"
