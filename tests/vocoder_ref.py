"""float64 reference of the vocoder's channel-last conv kernels (csrc/fo_vocoder.hip), the case tables the CPU and
GPU tests share, and the runners that launch a case through fo.ops and compare every output element.

Inputs: weights are bf16-representable (the packer's f2bf is exact, the reference uses the same numbers);
activations, biases and residuals are fp32 normals of both signs.

Error bound per output element (derived, not tuned).  With
    A = |oscale| * (sum |w| |x'| + |bias| + |res| + |res2|) + |gadd|      (float64)
and Ktot the number of products accumulated into the element (taps x Cin, over all members of a summed launch):
    E = (2^-18 + (2 Ktot + 8) 2^-23) A
2^-18 is the residual of the bf16 hi + lo split of an activation (two roundings of 2^-9; bf16 x bf16 products are
exact in fp32).  (Ktot + 8) 2^-24 A would bound Ktot fp32 accumulations plus the epilogue's few adds at one IEEE
rounding each; it is doubled because the MFMA's internal summation order and rounding are not documented as that.
The pair step propagates c1's bound through |w2| (leaky ReLU is 1-Lipschitz) and adds c2's own; tanh is
1-Lipschitz, so conv_post uses the same form.

Run as a program (one fresh process per FO_CONV_* setting, tests/test_vocoder_kernels_gpu.py) it checks the
conv_cl and pair tables and the small engine against the oracle, and exits non-zero on a mismatch.
"""
import math
import os
import sys
import zlib
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.1
SLOPE32 = float(np.float32(SLOPE))   # the value the kernels multiply by
SENT = 12345.678                     # sentinel of guard rows and positions no launch may write
THIRD = float(np.float32(1.0 / 3.0))


def coef(ktot):
    return 2.0 ** -18 + (2 * ktot + 8) * 2.0 ** -23


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def acts(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def weights(g, shape, ktot):
    """bf16-representable fp32 weights, scaled so that outputs stay O(1)."""
    return (torch.randn(*shape, generator=g, dtype=torch.float32) / math.sqrt(ktot)).bfloat16().float()


def leaky(x):
    return torch.where(x < 0, x * SLOPE32, x)


def conv64(x, w, dil, pad, Tq):
    """x [B][Tin][Cin], w [Cout][Cin][K] (float64) -> y [B][Tq][Cout], y[q] = sum_{j,ci} w[co][ci][j] *
    x[q + j*dil - pad][ci] with zeros outside [0, Tin)."""
    B, Tin, Cin = x.shape
    n = Tq + dil * (w.shape[-1] - 1)
    xw = x.new_zeros(B, Cin, n)                 # time steps -pad .. -pad + n - 1
    a, b = max(-pad, 0), min(n - pad, Tin)
    if b > a:
        xw[:, :, a + pad:b + pad] = x[:, a:b].transpose(1, 2)
    return F.conv1d(xw, w, dilation=dil).transpose(1, 2)


def _late(s, Tq, tw):
    """Mutation (b): outputs in the first 16 rows after a time-tile boundary take the next row's window."""
    idx = torch.tensor([q for q in range(Tq) if q >= tw and q % tw < 16], dtype=torch.long)
    out = s[:, :Tq].clone()
    if len(idx):
        out[:, idx] = s[:, idx + 1]
    return out


# ------------------------------------------------------------------------------------------------ conv_cl
def conv_member(g, B, Cin, Cout, K, dil, T, pre=True, bias=True, res=False, res2=False, oscale=1.0, gadd=False,
                cut=0):
    """One convolution with 'same' padding on T steps; cut > 0: Tq shorter than the natural length."""
    Tq = T - cut
    return NS(x=acts(g, B, T, Cin), w=weights(g, (Cout, Cin, K), K * Cin), bias=acts(g, Cout) if bias else None,
              K=K, dil=dil, pad=dil * (K - 1) // 2, Tq=Tq, Tout=T, ostride=1, ooff=0, pre=pre,
              res=acts(g, B, Tq, Cout) if res else None, res2=acts(g, B, Tq, Cout) if res2 else None,
              oscale=float(np.float32(oscale)), gadd=acts(g, B, Cout) if gadd else None, out_key=None)


def _conv_terms(m, mut, tw):
    x, w = m.x.double(), m.w.double()
    if "tap" in mut:
        w = w.clone()
        w[..., m.K - 1] = 0
    if m.pre and "leaky" not in mut:
        x = leaky(x)
    xa = x.abs()
    if "bf16" in mut:
        x = x.float().bfloat16().double()
    if "late" in mut:
        s = _late(conv64(x, w, m.dil, m.pad, m.Tq + 1), m.Tq, tw)
    else:
        s = conv64(x, w, m.dil, m.pad, m.Tq)
    a = conv64(xa, m.w.double().abs(), m.dil, m.pad, m.Tq)
    if m.bias is not None:
        a = a + m.bias.double().abs()
        if "bias" not in mut:
            s = s + m.bias.double()
    if m.res is not None:
        s, a = s + m.res.double(), a + m.res.double().abs()
    if m.res2 is not None:
        a = a + m.res2.double().abs()
        if "res2" not in mut:
            s = s + m.res2.double()
    return s, a


def conv_ref(members, summed=False, mut=(), tw=None):
    """-> [(y, E)] per output ([B][Tq][Cout] float64): one per member, or one for a summed launch (the output
    range, oscale and gadd are members[0]'s)."""
    outs = []
    for grp in ([members] if summed else [[m] for m in members]):
        s = a = 0.0
        ktot = 0
        for m in grp:
            si, ai = _conv_terms(m, mut, tw)
            s, a, ktot = s + si, a + ai, ktot + m.K * m.x.shape[2]
        m0 = grp[0]
        y, A = s * (1.0 if "oscale" in mut else m0.oscale), a * abs(m0.oscale)
        if m0.gadd is not None:
            A = A + m0.gadd.double().abs()[:, None]
            if "gadd" not in mut:
                y = y + m0.gadd.double()[:, None]
        outs.append((y, coef(ktot) * A))
    return outs


# ------------------------------------------------------------------------------------------------ pair step
def pair_member(g, B, C, K, dil, T):
    return NS(x=acts(g, B, T, C), w1=weights(g, (C, C, K), K * C), b1=acts(g, C), w2=weights(g, (C, C, K), K * C),
              b2=acts(g, C), K=K, dil=dil)


def _pair_terms(m, T, mut, tw):
    """y = x + c2(leaky(c1(leaky(x)))), c2 zero-padding c1's output outside [0, T)
    -> (y, A2, c1's bound through |w2|)"""
    x, w1, w2 = m.x.double(), m.w1.double(), m.w2.double()
    K, C = m.K, x.shape[2]
    p1, p2 = m.dil * (K - 1) // 2, (K - 1) // 2
    b1, b2 = (0.0, 0.0) if "bias" in mut else (m.b1.double(), m.b2.double())
    if "tap" in mut:
        w1, w2 = w1.clone(), w2.clone()
        w1[..., K - 1] = 0
        w2[..., K - 1] = 0
    lk = (lambda v: v) if "leaky" in mut else leaky
    rnd = (lambda v: v.float().bfloat16().double()) if "bf16" in mut else (lambda v: v)
    xa = lk(x)
    if "nozero" in mut:   # mutation (f): c1 evaluated, not zeroed, on the p2 rows either side of [0, T)
        u = rnd(lk(conv64(rnd(xa), w1, m.dil, p1 + p2, T + 2 * p2) + b1))
        c2 = conv64(u, w2, 1, 0, T)
    elif "late" in mut:
        c2 = _late(conv64(rnd(lk(conv64(rnd(xa), w1, m.dil, p1, T) + b1)), w2, 1, p2, T + 1), T, tw)
    else:
        c2 = conv64(rnd(lk(conv64(rnd(xa), w1, m.dil, p1, T) + b1)), w2, 1, p2, T)
    y = x + c2 + b2
    # the bound, always of the true computation
    xt = leaky(x)
    t1 = conv64(xt, m.w1.double(), m.dil, p1, T) + m.b1.double()
    E1 = coef(K * C) * (conv64(xt.abs(), m.w1.double().abs(), m.dil, p1, T) + m.b1.double().abs())
    A2 = conv64(leaky(t1).abs(), m.w2.double().abs(), 1, p2, T) + m.b2.double().abs() + x.abs()
    return y, A2, conv64(E1, m.w2.double().abs(), 1, p2, T)


def pair_ref(members, T, summed=False, oscale=1.0, gadd=None, mut=(), tw=None):
    """-> [(y, E)]: one per member, or one for a summed launch = (sum_g y_g) * oscale + gadd."""
    outs = []
    osc = float(np.float32(oscale))
    for grp in ([members] if summed else [[m] for m in members]):
        y = A = thru = 0.0
        ktot = 0
        for m in grp:
            yi, ai, ti = _pair_terms(m, T, mut, tw)
            y, A, thru, ktot = y + yi, A + ai, thru + ti, ktot + m.K * m.x.shape[2]
        y, A, thru = y * (1.0 if "oscale" in mut else osc), A * abs(osc), thru * abs(osc)
        if gadd is not None:
            A = A + gadd.double().abs()[:, None]
            if "gadd" not in mut:
                y = y + gadd.double()[:, None]
        outs.append((y, coef(ktot) * A + thru))
    return outs


# ------------------------------------------------------------------------------------------------ conv_post, polyphase
def post_ref(x, w, bias, K, pad):
    """x [B][T][C], w [1][C][K], bias [1] -> (tanh(conv(leaky(x)) + bias) [B][T], E)"""
    xa = leaky(x.double())
    T = x.shape[1] + 2 * pad - (K - 1)
    s = conv64(xa, w.double(), 1, pad, T) + bias.double()
    A = conv64(xa.abs(), w.double().abs(), 1, pad, T) + bias.double().abs()
    return torch.tanh(s)[..., 0], (coef(K * x.shape[2]) * A)[..., 0]


def convT_ref(x, W, bias, u, k):
    """float64 ConvTranspose1d(stride u, padding (k - u) // 2) of leaky(x): x [B][T][Cin], W [Cin][Cout][k]
    -> [B][Tout][Cout]"""
    y = F.conv_transpose1d(leaky(x.double()).transpose(1, 2), W.double(), bias.double(), stride=u,
                           padding=(k - u) // 2)
    return y.transpose(1, 2)


def poly_members(x, W, bias, u, k, phases):
    """The u stride-1 convolutions of a ConvTranspose1d from phases = [(r, j0, pad_r)] (CodecEngine.polyphase):
    phase r holds taps j0, j0 + u, ... reversed and writes time steps r, r + u, ... of one output."""
    Tin = x.shape[1]
    Tout = (Tin - 1) * u - 2 * ((k - u) // 2) + k
    ms = []
    for r, j0, pad_r in phases:
        K = (k - j0 + u - 1) // u
        w = torch.stack([W[:, :, j0 + u * (K - 1 - j)].t() for j in range(K)], dim=2).contiguous()
        ms.append(NS(x=x, w=w, bias=bias, K=K, dil=1, pad=pad_r, Tq=(Tout - r + u - 1) // u, Tout=Tout, ostride=u,
                     ooff=r, pre=True, res=None, res2=None, oscale=1.0, gadd=None, out_key="up", j0=j0))
    return ms


def interleave(members, outs):
    """Per-member results [B][Tq][Cout] -> the strided output [B][Tout][Cout] (NaN where no member writes)."""
    m0 = members[0]
    full = torch.full((outs[0].shape[0], m0.Tout, outs[0].shape[2]), float("nan"), dtype=torch.float64)
    for m, o in zip(members, outs):
        full[:, m.ooff::m.ostride][:, :m.Tq] = o
    return full


# ------------------------------------------------------------------------------------------------ case tables
# k_conv_cl instantiation <MTW, NTW, CK> by conv_launch's rules at the default chunk width:
#   CK  = 32 for Cin >= 32, else 16
#   MTW = Cout / 16 for Cout <= 32 (NTW = 8 / MTW), 4 for Cout >= 64 (NTW = 2) -- unless the grid
#         ceil(Tq_max / 128) * (Cout / 64) * B * (1 if summed else G) is below 256 workgroups: then <2, 2, CK>
#   time tile TW = 64 NTW
#   instantiation  Cin  Cout   TW   cases
#   <1,8,16>        16    16  512   cl/<1,8,16>/*
#   <1,8,32>        64    16  512   cl/<1,8,32>/*, multi/sum*
#   <2,4,16>        16    32  256   cl/<2,4,16>/*
#   <2,4,32>        64    32  256   cl/<2,4,32>/*, multi/u1, multi/u3
#   <2,2,16>        16   128  128   cl/<2,2,16>/*, multi/u5           (grids of 6 .. 24 workgroups)
#   <2,2,32>        64   128  128   cl/<2,2,32>/*
#   <4,2,16>        16   128  128   big/<4,2,16>/u (B 2, 4 members, Tq_max 1930: 16 * 2 * 2 * 4 = 256 workgroups)
#                   16   256        big/<4,2,16>/sum (B 4, summed:            16 * 4 * 4     = 256)
#   <4,2,32>        64   128/256    big/<4,2,32>/u, big/<4,2,32>/sum
# Options (every one in all six small-grid instantiations; the big ones carry all four as members):
#   edge   (11,5) on TW + 37 steps: 50-row halo across the tile boundary, partial second tile
#   short  (3,1) on 5 steps, no leaky, null bias, res only
#   epi    (7,3) on TW + 37 steps, res, res2 aliasing out, oscale 1/3, per-row gadd, Tq 3 short of the natural length
#   short5 (3,1) on 5 steps with leaky and bias (5 steps are shorter than the halo; with wider kernels the outer
#          taps would meet nothing but padding, and a dropped tap could not show)
SMALL = [("<1,8,16>", 16, 16, 512), ("<1,8,32>", 64, 16, 512), ("<2,4,16>", 16, 32, 256), ("<2,4,32>", 64, 32, 256),
         ("<2,2,16>", 16, 128, 128), ("<2,2,32>", 64, 128, 128)]
OPTS = {"edge": dict(K=11, dil=5), "short": dict(K=3, dil=1, T=5, pre=False, bias=False, res=True),
        "epi": dict(K=7, dil=3, res=True, res2=True, oscale=THIRD, gadd=True, cut=3), "short5": dict(K=3, dil=1, T=5)}


def _mk(name, family, Cin, Cout, B, specs, tw, api="multi", summed=False, inst=None):
    def build():
        g = gen(name)
        return [conv_member(g, B, Cin, Cout, **s) for s in specs]
    return NS(name=name, family=family, Cin=Cin, Cout=Cout, B=B, build=build, tw=tw, api=api, summed=summed, inst=inst)


def _opt(o, tw, T=None):
    s = dict(OPTS[o])
    s.setdefault("T", T or tw + 37)
    return s


CONV_CASES = [_mk(f"cl/{inst}/{o}", "conv_cl", Cin, Cout, 3, [_opt(o, tw)], tw, api="cl", inst=inst)
              for inst, Cin, Cout, tw in SMALL for o in OPTS]
# (summed launches take oscale and gadd from member 0: the other members carry values that must be ignored)
_SUM3 = [dict(K=K, dil=d, T=1930, res=True, oscale=0.5 if i else THIRD, gadd=True)
         for i, (K, d) in enumerate(((3, 1), (7, 3), (11, 5)))]
for _inst, _cin in (("<4,2,16>", 16), ("<4,2,32>", 64)):
    CONV_CASES.append(_mk(f"big/{_inst}/u", "conv_cl", _cin, 128, 2,
                          [_opt("edge", 128, T=1930), _opt("short", 128), _opt("epi", 128), _opt("short5", 128)],
                          128, inst=_inst))
    CONV_CASES.append(_mk(f"big/{_inst}/sum", "conv_cl", _cin, 256, 4, _SUM3, 128, summed=True, inst=_inst))

_KD5 = [(3, 1), (5, 2), (7, 3), (9, 1), (11, 5)]
MULTI_CASES = [
    _mk("multi/u1", "multi", 64, 32, 3, [dict(K=7, dil=3, T=293)], 256),
    _mk("multi/u3", "multi", 64, 32, 3, [dict(K=7, dil=3, T=293), dict(K=3, dil=1, T=5, res=True),
                                        dict(K=11, dil=5, T=100, pre=False)], 256),
    _mk("multi/u5", "multi", 16, 128, 3, [dict(K=K, dil=d, T=T, bias=bool(i % 2), res2=i == 2)
                                         for i, ((K, d), T) in enumerate(zip(_KD5, (165, 5, 130, 64, 140)))], 128),
] + [_mk(f"multi/sum{G}", "multi", 64, 16, 3, [dict(K=K, dil=d, T=549, res=True, oscale=0.5 if i else THIRD, gadd=True)
                                               for i, (K, d) in enumerate(_KD5[:G])], 512, summed=True)
     for G in (1, 3, 5)]

# k_conv_pair instantiation by channel count: C 16 <1,4,16> (TW 256), C 32 <2,2,32> (TW 128), C 64 <4,2,32> (TW 128)
PAIR_KD = [(3, 1), (7, 3), (11, 5)]
PAIR_TW = {16: 256, 32: 128, 64: 128}


def _mkp(C, T, kds, summed):
    name = f"pair/C{C}/T{T}/G{len(kds)}{'s' if summed else 'u'}" + (f"/K{kds[0][0]}" if len(kds) == 1 else "")

    def build():
        g = gen(name)
        ms = [pair_member(g, 3, C, K, d, T) for K, d in kds]
        return ms, (acts(g, 3, C) if summed else None)
    return NS(name=name, family="pair", C=C, T=T, B=3, build=build, summed=summed, tw=PAIR_TW[C],
              oscale=THIRD if summed else 1.0)


# (on 5 steps the members are (3,1) and (7,3): the outer taps of an 11-tap kernel would meet nothing but padding)
PAIR_CASES = [_mkp(C, T, kds, summed) for C in (16, 32, 64) for T in (5, PAIR_TW[C] + 9, 2 * PAIR_TW[C])
              for kds, summed in (((PAIR_KD, False), (PAIR_KD, True), (PAIR_KD[2:], False), (PAIR_KD[1:2], True))
                                  if T > 5 else ((PAIR_KD[:2] + PAIR_KD[:1], False), (PAIR_KD[:2] + PAIR_KD[:1], True),
                                                 (PAIR_KD[:1], False), (PAIR_KD[1:2], True)))]

POLY_UK = [(5, 10), (4, 8), (3, 6), (2, 4), (2, 5), (3, 8)]


def poly_case(u, k, Cin, Tin, phases):
    g = gen(f"poly/{u}/{k}/{Cin}/{Tin}")
    x, W, b = acts(g, 2, Tin, Cin), weights(g, (Cin, Cin // 2, k), Cin * k // u), acts(g, Cin // 2)
    return x, W, b, poly_members(x, W, b, u, k, phases)


def pair_refused(C):
    """Channel counts fo_conv_pair_multi refuses under a non-default FO_CONV_CK (it is built for chunks of 32
    channels, 16 for C = 16)."""
    ck = os.environ.get("FO_CONV_CK")
    return (ck == "16" and C >= 32) or (ck == "64" and C >= 64)


# ------------------------------------------------------------------------------------------------ GPU runners
OBSERVED = {}   # family -> greatest err / E seen


def note(family, r):
    OBSERVED[family] = max(OBSERVED.get(family, 0.0), r)
    return r


class Guarded:
    """A [B][T][C] fp32 device tensor inside a sentinel-filled allocation with 8 guard rows either side."""

    def __init__(self, B, T, C, dev):
        self.g = 8 * C
        self.full = torch.full((2 * self.g + B * T * C,), SENT, dtype=torch.float32, device=dev)
        self.t = self.full[self.g:self.g + B * T * C].view(B, T, C)
        self.mask = torch.zeros(B, T, C, dtype=torch.bool)   # what a launch is expected to write
        self.init = None

    def arm(self):
        self.init = self.full.cpu().clone()

    def check(self, what):
        """Everything outside the mask came back bit-identical."""
        got = self.full.cpu()
        keep = torch.ones(got.shape, dtype=torch.bool)
        keep[self.g:-self.g] = ~self.mask.view(-1)
        assert torch.equal(got.view(torch.int32)[keep], self.init.view(torch.int32)[keep]), \
            f"{what}: a guard row or an unwritten position changed"
        return got[self.g:-self.g].view(self.mask.shape)


def ratio(got, y, E):
    err = (got.double() - y).abs()
    assert torch.isfinite(err).all()
    return float(torch.where(err == 0, torch.zeros_like(err), err / E).max())


def pos(m):
    return slice(m.ooff, m.ooff + (m.Tq - 1) * m.ostride + 1, m.ostride)


def launch_conv(ops, members, B, Cin, Cout, dev, api, summed, pcs=None):
    """Launch members (one conv_cl each for api 'cl', else one conv_cl_multi) -> {out key: Guarded}, armed and
    launched but not yet checked."""
    outs, descs = {}, []
    for i, m in enumerate(members):
        key = 0 if summed else (i if m.out_key is None else m.out_key)
        if key not in outs:
            outs[key] = Guarded(B, m.Tout, Cout, dev)
        o = outs[key]
        o.mask[:, pos(m)] = True
        res = res2 = None
        if m.res is not None:
            res = torch.zeros(B, m.Tout, Cout, device=dev)
            res[:, pos(m)] = m.res.to(dev)
        if m.res2 is not None:   # res2 aliases out: the launch reads its own output positions
            o.t[:, pos(m)] = m.res2.to(dev)
            res2 = o.t
        pc = pcs[i] if pcs else ops.PackedConv(m.w.to(dev).bfloat16(), None if m.bias is None else m.bias.to(dev))
        kw = dict(Tq=m.Tq, ostride=m.ostride, ooff=m.ooff, Tout_total=m.Tout, pre_leaky=SLOPE if m.pre else None,
                  res=res, res2=res2, oscale=m.oscale, gadd=None if m.gadd is None else m.gadd.to(dev))
        descs.append((m.x.to(dev), m.x.shape[1], pc, m.dil, m.pad, o.t, kw))
    for o in outs.values():
        o.arm()
    if api == "cl":
        for x, Tin, pc, dil, pad, out, kw in descs:
            ops.conv_cl(x, B, Cin, Tin, pc, dil, pad, out, **kw)
    else:
        ops.conv_cl_multi([ops.conv_desc(x, Tin, pc, dil, pad, out, **kw) for x, Tin, pc, dil, pad, out, kw in descs],
                          B, Cin, Cout, dev, summed=summed)
    torch.cuda.synchronize(dev)
    return outs


def run_conv_case(case, dev):
    from fo import ops
    ms = case.build()
    refs = conv_ref(ms, case.summed)
    outs = launch_conv(ops, ms, case.B, case.Cin, case.Cout, dev, case.api, case.summed)
    worst = 0.0
    for i, (y, E) in enumerate(refs):
        got = outs[0 if case.summed else i].check(case.name)
        worst = max(worst, ratio(got[:, pos(ms[i])], y, E))
    return note(case.family, worst)


def run_pair_case(case, dev):
    from fo import ops
    ms, gadd = case.build()
    B, C, T = case.B, case.C, case.T
    refs = pair_ref(ms, T, case.summed, case.oscale, gadd)
    outs = [Guarded(B, T, C, dev) for _ in range(1 if case.summed else len(ms))]
    members = []
    for i, m in enumerate(ms):
        o = outs[0 if case.summed else i]
        o.mask[:] = True
        members.append((m.x.to(dev), ops.PackedConv(m.w1.to(dev).bfloat16(), m.b1.to(dev)),
                        ops.PackedConv(m.w2.to(dev).bfloat16(), m.b2.to(dev)), m.K, m.dil, o.t))
    for o in outs:
        o.arm()
    try:
        ops.conv_pair_multi(members, B, C, T, dev, slope=SLOPE, summed=case.summed, oscale=case.oscale,
                            gadd=None if gadd is None else gadd.to(dev))
    except RuntimeError:
        if not pair_refused(C):
            raise
        torch.cuda.synchronize(dev)
        for o in outs:   # a refusal writes nothing
            o.mask[:] = False
            o.check(case.name)
        return None
    assert not pair_refused(C), f"{case.name}: fo_conv_pair_multi documents this chunk width as refused"
    torch.cuda.synchronize(dev)
    return note("pair", max(ratio(o.check(case.name), y, E) for o, (y, E) in zip(outs, refs)))


# ------------------------------------------------------------------------------------------------ engine level
GST = [[3, 17, 41, 8, 22, 59, 0, 33], [5, 1, 40, 58, 0, 13, 27, 9]]


def engine_cfg():
    """A small ResBlock1 geometry whose stages are 128, 64, 32 and 16 channels wide: the gadd path (128), grouped
    conv_cl_multi launches with the summed last conv (128, 64) and the pair kernel (32, 16)."""
    from oracle import configs
    cfg = configs.get("tiny")
    cfg["codec_json"].update(upsample_initial_channel=256, upsample_rates=[2, 2, 2, 2],
                             upsample_kernel_sizes=[4, 4, 4, 4], resblock_kernel_sizes=[3, 7, 11],
                             resblock_dilation_sizes=[[1, 3, 5]] * 3, n_codes=60)
    return cfg


_ORACLE = {}


def engine_oracle():
    """(ids [2][40], the oracle's PCM per row with the row's own global style tokens), computed once."""
    if not _ORACLE:
        from oracle import nets
        from oracle.params import codec_shapes
        from oracle.weights import SynthCheckpoint
        cfg = engine_cfg()
        W = SynthCheckpoint(cfg["seed"], codec_shapes(cfg), cfg["overrides"])
        ids = np.random.default_rng(11).integers(0, 60, size=(2, 40))
        codec = nets.Codec(W, cfg)
        _ORACLE["v"] = (ids, np.stack([codec(ids[b], GST[b]) for b in range(2)]))
    return _ORACLE["v"]


def engine_check(dev, modes=("default", "pair=False", "grouped=False")):
    from fo.codec import CodecEngine
    from fo.weights import SynthSource
    from oracle.params import codec_shapes
    cfg = engine_cfg()
    ids, want = engine_oracle()
    src = SynthSource(cfg["seed"], codec_shapes(cfg), dev, cfg["overrides"])
    for mode in modes:
        eng = CodecEngine(src, cfg["codec_json"], dev)
        assert eng.grouped and eng.pair and [len(p) for p in eng.p_ups] == [2, 2, 2, 2]
        if mode == "pair=False":
            eng.pair = False
        elif mode == "grouped=False":
            eng.grouped = False
        pcm = eng(torch.from_numpy(ids).to(dev, torch.int32), gfeat=eng.global_feature(torch.tensor(GST), 2))
        assert pcm.shape == want.shape, (mode, pcm.shape, want.shape)
        np.testing.assert_allclose(pcm.cpu().numpy(), want, rtol=2e-3, atol=5e-5, err_msg=mode)
        eng.destroy()


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "freeze-omni_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    dev = torch.device("cuda:0")
    bad = []
    for case in CONV_CASES:
        r = run_conv_case(case, dev)
        if not r <= 1.0:
            bad.append((case.name, r))
    refused = 0
    for case in PAIR_CASES:
        r = run_pair_case(case, dev)
        refused += r is None
        if r is not None and not r <= 1.0:
            bad.append((case.name, r))
    engine_check(dev)
    print(f"vocoder_ref: {len(CONV_CASES)} conv and {len(PAIR_CASES)} pair cases ({refused} refused as documented), "
          f"max err/E {OBSERVED}, engine ok; mismatches: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
