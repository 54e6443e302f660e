"""float64 session model, derived error bound and case tables of the speech encoder's rel-pos attention kernels
(csrc/fo_attn.hip: k_relpos_fused, k_relpos_chunks + k_relpos_chunks_append, k_relpos_attn + k_enc_kv_write).  No GPU
import: tests/test_relpos_ref_cpu.py shows on the CPU that the bound rejects wrong kernels and wrong ring bookkeeping
and that every condition on the inputs holds; tests/test_relpos_kernels_gpu.py launches the cases through fo.ops
between guards.

Model (MultiHeadedAttention.infer, models/encoder/attention.py:407-459, and RelPositionalEncoding.infer, :105-121, of
the reference).  A session holds the K and V rows it keeps ([n][d], float64) and its pe.  step(q, k, v): the context
is the held rows followed by the chunk's rows (Lk rows), P = ptab[p0 : p0 + Lk] with p0 = max(0, pe % max_len -
full_chunk), per head softmax(((q + bu) K^T + (q + bv) P^T) * float32(scale)) V; afterwards the session holds the
last buffersize rows of the context and pe = pe % max_len + chunk.  No start, length, modulo or slot arithmetic
appears in it: that arithmetic (SpeechEncoderEngine.host_meta / advance and the kernels' ring indexing) is what is
under test.  ptab stands for linear_pos(sinusoid(position)); a random table is as good a stand-in for the kernels.

Bound E per output element, in helper_ref's notation (U = 2^-24, gam(k) bounds k roundings in a chain, SECOND covers
products of first-order terms).  With qu = q + bu, qv = q + bv, ac = qu . K_j, bd = qv . P_j, s_j = (ac + bd) scale
(scale the float32 value the launch receives), M = max_j s_j and w_j = exp(s_j - M) / sum_k exp(s_k - M):
  score     q + b rounds once and a dk-term float32 dot product in any summation order, fused or not, adds gam(dk):
            gam(dk + 1) A_j with A_j = |qu| . |K_j| + |qv| . |P_j|; the addition ac + bd and the product by scale
            round once each:
                ds_j = scale (gam(dk + 1) A_j + 2 U |ac + bd|) SECOND
  exponent  the kernel subtracts its own maximum m^ of its own scores; a softmax does not depend on the shift, so
            only the rounding of s^_j - m^ counts, U |s^_j - m^| <= U ((M - s_j) + ds_j + D) =: dl_j with D = max_k
            ds_k (m^ lies within D of M)
  expf      the device expf, relative EXPF = 2^-22 (sampler_ref.EXPF, with the reason given there), plus TINY =
            2^-126 absolute where it underflows (the greatest term is expf(0) = 1, so TINY is relative to the sum too):
                e_j = C exp(s_j - M) (1 + r_j),  |r_j| <= rho_j = exp(ds_j + dl_j) (1 + EXPF) - 1
  sum       each lane adds its ceil(Lk / 64) terms in turn, then 6 butterfly levels: g = gam(ceil(Lk / 64) + 6);
            sum^ = C sum_k exp(s_k - M) (1 + r_k)(1 + h_k), |h_k| <= g, so sum^ / (C Z) = 1 + th with
                |th| <= TH = sum_k w_k (rho_k + g + rho_k g) + Lk TINY
  weight    r = 1 / sum^ (a division: 2 U) and e_j r (U):
                dw_j = w_j ((1 + rho_j)(1 + 3 U) / (1 - TH) - 1) + TINY
  P.V       a sequential Lk-term sum of products (a term passes its product and at most Lk - 1 additions):
                E_c = sum_j dw_j |V_jc| + gam(Lk) sum_j (w_j + dw_j) |V_jc|
The ring appends are copies: ring contents are compared with torch.equal.
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

from helper_ref import OBSERVED, SECOND, U, Guard, gam, gen, note, randn, ratio  # noqa: F401  (some for the tests)
from sampler_ref import EXPF

TINY = 2.0 ** -126
CEIL = 2e-4          # tests/test_enc_block_gpu.py grants the fused block 2e-4 max|x|: the bound stays below it
MUT_MODEL = ("pshift", "buvswap", "scale_ac", "phead0")
MUT_RING = ("slotb", "trim-1", "trim+1", "late")       # these write or keep other rows: the ring state differs too
MUTANTS = MUT_MODEL + MUT_RING + ("nowrap", "noown")    # (these two only read other rows)


def scale_of(dk):
    return float(np.float32(1.0 / math.sqrt(dk)))


def attend(q, K, V, P, bu, bv, h, dk, scale, mut=()):
    """q [T][d] float32, K / V / P [Lk][d] float64, bu / bv [d] -> (y, E) [T][d] float64 (see the docstring)"""
    T, d = q.shape
    Lk = K.shape[0]
    if Lk == 0:
        return torch.full((T, d), math.nan, dtype=torch.float64), torch.zeros(T, d, dtype=torch.float64)
    q64 = q.double()
    y = torch.zeros(T, d, dtype=torch.float64)
    E = torch.zeros(T, d, dtype=torch.float64)
    g = gam(-(-Lk // 64) + 6)
    b1, b2 = (bv, bu) if "buvswap" in mut else (bu, bv)
    for hh in range(h):
        sl = slice(hh * dk, (hh + 1) * dk)
        psl = slice(0, dk) if "phead0" in mut else sl
        qu, qv = q64[:, sl] + b1[sl].double(), q64[:, sl] + b2[sl].double()
        Kh, Ph, Vh = K[:, sl], P[:, psl], V[:, sl]
        ac, bd = qu @ Kh.t(), qv @ Ph.t()
        s = ac * scale + bd if "scale_ac" in mut else (ac + bd) * scale
        A = qu.abs() @ Kh.abs().t() + qv.abs() @ Ph.abs().t()
        ds = scale * (gam(dk + 1) * A + 2 * U * (ac + bd).abs()) * SECOND
        M = s.max(-1, keepdim=True).values
        w = torch.softmax(s, -1)
        dl = U * ((M - s) + ds + ds.max(-1, keepdim=True).values)
        rho = torch.exp(ds + dl) * (1 + EXPF) - 1
        TH = (w * (rho + g + rho * g)).sum(-1, keepdim=True) + Lk * TINY
        dw = w * ((1 + rho) * (1 + 3 * U) / (1 - TH) - 1) + TINY
        y[:, sl] = w @ Vh
        E[:, sl] = dw @ Vh.abs() + gam(Lk) * ((w + dw) @ Vh.abs())
    return y, E


class Session:
    def __init__(self, pe, K=None, V=None, d=0):
        self.pe = pe
        self.K = torch.zeros(0, d, dtype=torch.float64) if K is None else K.double().clone()
        self.V = torch.zeros(0, d, dtype=torch.float64) if V is None else V.double().clone()


class Model:
    def __init__(self, ptab, bu, bv, h, dk, chunk, buffersize, full_chunk, max_len):
        self.ptab, self.bu, self.bv, self.h, self.dk = ptab.double(), bu, bv, h, dk
        self.chunk, self.buffersize, self.full_chunk, self.max_len = chunk, buffersize, full_chunk, max_len
        self.scale = scale_of(dk)

    def step(self, s, q, k, v, mut=()):
        """q, k, v float32 [T][d] -> (y, E) [T][d]; the session moves on"""
        K, V = torch.cat([s.K, k.double()]), torch.cat([s.V, v.double()])
        Lk = K.shape[0]
        p0 = max(0, s.pe % self.max_len - self.full_chunk) + (1 if "pshift" in mut else 0)
        y, E = attend(q, K, V, self.ptab[p0:p0 + Lk], self.bu, self.bv, self.h, self.dk, self.scale, mut)
        s.K, s.V = K[-self.buffersize:], V[-self.buffersize:]
        s.pe = s.pe % self.max_len + self.chunk
        return y, E


# ------------------------------------------------------------------------------------------------ a CPU ring
def launch_cpu(qkv, kr, vr, cap, start, length, ring, ptab, pstart, bu, bv, B, T, h, dk, scale, mut=()):
    """fo_relpos_attention_fused restated on CPU tensors with the kernels' ring arithmetic (float64 sums, the output
    rounded to float32 like a kernel's): kr / vr [slots][cap][d] are appended to in place -> out [B T][d] float32.
    mut: a wrong kernel -- "slotb" slot b instead of ring[b], "nowrap" (start + j) without % cap (the rows run on
    into the next slot), "noown" the chunk's own rows left out of its context, "late" the append one slot late,
    and attend()'s."""
    d = h * dk
    krf, vrf = kr.view(-1, d), vr.view(-1, d)
    out = torch.empty(B * T, d, dtype=torch.float32)
    for b in range(B):
        rb = b if ring is None or "slotb" in mut else int(ring[b])
        st, ln, ps = int(start[b]), int(length[b]), int(pstart[b]) + (1 if "pshift" in mut else 0)
        rows = [rb * cap + ((st + j) if "nowrap" in mut else (st + j) % cap) for j in range(ln)]
        r = qkv[b * T:(b + 1) * T]
        q, k, v = r[:, :d], r[:, d:2 * d], r[:, 2 * d:3 * d]
        own = "noown" not in mut
        K = torch.cat([krf[rows].double()] + ([k.double()] if own else []))
        V = torch.cat([vrf[rows].double()] + ([v.double()] if own else []))
        y, _ = attend(q, K, V, ptab[ps:ps + K.shape[0]].double(), bu, bv, h, dk, scale, mut)
        out[b * T:(b + 1) * T] = y.float()
        for t in range(T):
            at = rb * cap + (st + ln + t + (1 if "late" in mut else 0)) % cap
            krf[at], vrf[at] = k[t], v[t]
    return out


def live_rows(ring, slot, start, length, cap):
    """the rows a session holds, oldest first, as the ring has them"""
    return ring[slot][[(start + j) % cap for j in range(length)]]


# ------------------------------------------------------------------------------------------------ single launches
# Metadata given directly.  Starts wrap (start = cap - 2 - 3 b: every context of 3 rows or more runs over the ring's
# end), ring slots are a permutation of B + 3 slots, pstart is distinct per session and 0 for session 0.
PSTART = [0, 17, 5, 40, 3, 29, 11, 8]
FC1 = 68             # the single-launch model's full_chunk: pe = pstart + FC1 (31 where pstart is 0, below FC1)


def _single(name, dk, h, cap, B, T, lens, ring=True, tight=False, kind=None):
    d = h * dk
    assert len(lens) == B and max(lens) + T <= cap
    slots = B + 3 if ring else B
    start = [(cap - 2 - 3 * b) % cap for b in range(B)]
    pstart = [3, 90] if kind == "peaked" else PSTART[:B]
    npos = max(pstart) + max(lens) + T + 5

    def build():
        g = gen("relpos/" + name)
        rg = [int(i) for i in torch.randperm(slots, generator=g)[:B]] if ring else None
        qkv = randn(g, B * T, 3 * d)
        ptab = randn(g, npos, d)
        K0 = [randn(g, n, d) for n in lens]
        V0 = [randn(g, n, d) for n in lens]
        if kind == "peaked":
            qkv[:T, :d] *= 8.0                                   # session 0: the max subtraction carries the result
            key = randn(g, d)
            K0[1][:] = key                                       # session 1: every key and position row identical:
            qkv[T:2 * T, d:2 * d] = key                          # uniform weights, the output is the mean of V
            ptab[pstart[1]:pstart[1] + lens[1] + T] = randn(g, d)
        kr, vr = randn(g, slots, cap, d), randn(g, slots, cap, d)   # (the rows no session holds: noise)
        for b in range(B):
            at = [(start[b] + j) % cap for j in range(lens[b])]
            kr[rg[b] if ring else b][at] = K0[b]
            vr[rg[b] if ring else b][at] = V0[b]
        return NS(qkv=qkv, ptab=ptab, K0=K0, V0=V0, kr=kr, vr=vr, ring=rg, bu=0.3 * randn(g, d), bv=0.3 * randn(g, d))
    return NS(name=name, dk=dk, h=h, d=d, cap=cap, B=B, T=T, lens=lens, slots=slots, start=start, pstart=pstart,
              npos=npos, ldq=3 * d + (0 if tight else 32), ldo=d + (0 if tight else 16), scale=scale_of(dk),
              kind=kind, build=build)


SINGLE_CASES = [
    _single("real7", 64, 16, 72, 8, 7, [64, 0, 13, 64, 57, 5, 64, 1]),
    _single("full8", 64, 4, 72, 3, 8, [64, 64, 0]),
    _single("one", 64, 4, 72, 5, 1, [0, 1, 2, 63, 64]),
    _single("tiny", 8, 4, 16, 3, 4, [8, 3, 0], tight=True),
    _single("tail9", 64, 2, 72, 2, 9, [63, 10]),
    _single("wide", 64, 2, 144, 2, 8, [130, 7]),
    _single("noring", 64, 4, 72, 3, 4, [0, 37, 64], ring=False),
    _single("peaked", 64, 4, 72, 2, 7, [64, 20], kind="peaked"),
]
_SINGLE = {}


def single_ref(case, mut=()):
    """-> (data, y [B T][d], E, held: per session the (K, V) the model holds afterwards); cached for mut == ()"""
    if not mut and case.name in _SINGLE:
        return _SINGLE[case.name]
    data = _SINGLE[case.name][0] if case.name in _SINGLE else case.build()
    m = Model(data.ptab, data.bu, data.bv, case.h, case.dk, 4, case.cap - 8, FC1, 10 ** 6)
    ys, Es, held = [], [], []
    d, T = case.d, case.T
    for b in range(case.B):
        s = Session(case.pstart[b] + FC1 if case.pstart[b] else 31, data.K0[b], data.V0[b], d)
        r = data.qkv[b * T:(b + 1) * T]
        y, E = m.step(s, r[:, :d], r[:, d:2 * d], r[:, 2 * d:], mut)
        ys.append(y)
        Es.append(E)
        held.append((s.K, s.V))
    res = (data, torch.cat(ys), torch.cat(Es), held)
    if not mut:
        _SINGLE[case.name] = res
    return res


def single_cpu(case, mut=()):
    """the case through launch_cpu on a copy of its rings -> (out float32, kr, vr)"""
    data = single_ref(case)[0]
    kr, vr = data.kr.clone(), data.vr.clone()
    if "nowrap" in mut:       # a slot of noise behind the last one for the rows that run on
        kr, vr = torch.cat([kr, kr[:1] + 1.0]), torch.cat([vr, vr[:1] + 1.0])
    out = launch_cpu(data.qkv, kr, vr, case.cap, case.start, case.lens, data.ring, data.ptab, case.pstart, data.bu,
                     data.bv, case.B, case.T, case.h, case.dk, case.scale, mut)
    return out, kr, vr


def after_advance(case, b):
    """(start, len) of session b after the chunk, by advance()'s rule with buffersize = cap - 8"""
    total = case.lens[b] + case.T
    keep = min(total, case.cap - 8)
    return (case.start[b] + total - keep) % case.cap, keep


# ------------------------------------------------------------------------------------------------ sequences
# Four sessions over `steps` chunks; all ring / position metadata comes from SpeechEncoderEngine.host_meta / advance,
# called unbound on stub().  Session i takes part from step join[i] on, starting with init[i] = (len, start) rows
# already held (a cache handed over mid-stream) and pe[i]; its ring slot is SLOT[i] of NSLOT.
SLOT, NSLOT = [5, 2, 0, 3], 6


def _seq(name, dk, h, chunk, left, T, steps, join, init, pe):
    d = h * dk
    bs, fc = chunk * left, chunk * (left + 1)
    max_len = chunk * (300 // chunk) - fc
    cap = bs + 8

    def stub():
        return NS(chunk=chunk, left=left, buffersize=bs, full_chunk=fc, max_len=max_len, cap=cap)

    def build():
        g = gen("relpos/" + name)
        return NS(ptab=randn(g, max_len, d), bu=0.3 * randn(g, d), bv=0.3 * randn(g, d),
                  qkv=randn(g, steps, 4, T, 3 * d), K0=[randn(g, n, d) for n, _ in init],
                  V0=[randn(g, n, d) for n, _ in init], kr=randn(g, NSLOT, cap, d), vr=randn(g, NSLOT, cap, d))
    return NS(name=name, dk=dk, h=h, d=d, chunk=chunk, left=left, T=T, steps=steps, join=join, init=init, pe=pe,
              cap=cap, max_len=max_len, buffersize=bs, full_chunk=fc, scale=scale_of(dk), stub=stub, build=build)


SEQ_CASES = [
    # session 0 is handed over with 60 rows (full after its first chunk, trimmed from its second on) and wraps
    # pe % max_len (232) at step 7 with a full ring; 1 starts empty beside it; 2 joins empty at step 5; 3 joins at
    # step 11 with a full ring and a pe two turns up that wraps at once.  Largest row read: pe - 1 <= max_len - 2.
    _seq("seq_real", 64, 4, 4, 16, 4, 20, [0, 0, 5, 11], [(60, 65), (0, 0), (0, 70), (64, 71)],
         [207, 0, 50, 2 * 232 + 230]),
    # T = 7: pe a multiple of 4 and at most 224 (largest row read pe + 2)
    _seq("seq_b", 64, 4, 4, 16, 7, 12, [0, 0, 2, 4], [(57, 68), (0, 3), (0, 0), (64, 40)], [0, 40, 100, 180]),
    # cap 16 = 4 chunks of 4 rows; session 0 wraps pe % max_len (288) at step 3 with a full ring
    _seq("seq_tiny", 8, 4, 4, 2, 4, 8, [0, 0, 2, 4], [(8, 13), (0, 0), (0, 15), (5, 9)], [278, 0, 24, 288 + 284]),
]
_SEQ = {}


def active(case, step):
    return [i for i in range(4) if case.join[i] <= step]


def seq_ref(case):
    """-> (data, out: per step {session: (y, E)}, held: per step {session: (K, V)} after it); cached"""
    if case.name not in _SEQ:
        data = case.build()
        m = Model(data.ptab, data.bu, data.bv, case.h, case.dk, case.chunk, case.buffersize, case.full_chunk,
                  case.max_len)
        sess = [Session(case.pe[i], data.K0[i], data.V0[i], case.d) for i in range(4)]
        d, out, held = case.d, [], []
        for st in range(case.steps):
            o = {}
            for i in active(case, st):
                r = data.qkv[st, i]
                o[i] = m.step(sess[i], r[:, :d], r[:, d:2 * d], r[:, 2 * d:])
            out.append(o)
            held.append({i: (sess[i].K, sess[i].V) for i in active(case, st)})
        _SEQ[case.name] = (data, out, held)
    return _SEQ[case.name]


def new_caches(case, data, kr, vr):
    """the four sessions' caches (start, len, slot) with their handed-over rows placed in the rings"""
    caches = []
    for i, (n, st) in enumerate(case.init):
        at = [(st + j) % case.cap for j in range(n)]
        kr[SLOT[i]][at] = data.K0[i].to(kr.device)
        vr[SLOT[i]][at] = data.V0[i].to(vr.device)
        caches.append(NS(start=st, len=n, slot=SLOT[i]))
    return caches


def groups(case, C):
    """the steps in runs of at most C with the same sessions taking part: [(first step, count)]"""
    out, st = [], 0
    while st < case.steps:
        n = 1
        while n < C and st + n < case.steps and active(case, st + n) == active(case, st):
            n += 1
        out.append((st, n))
        st += n
    return out


def seq_cpu(case, engine_cls, mut=()):
    """The sequence on a CPU ring, driven by engine_cls.host_meta / advance on the stub -> (out: per step {session:
    float32 [T][d]}, live: per step {session: (K rows, V rows)} as the ring holds them).  mut "trim-1" / "trim+1":
    advance keeps one row fewer / more."""
    data = seq_ref(case)[0]
    stub, adv = case.stub(), case.stub()
    adv.buffersize += {"trim-1": -1, "trim+1": 1}.get(mut if isinstance(mut, str) else "", 0)
    extra = 1 if "nowrap" in mut else 0
    kr = torch.cat([data.kr, data.kr[:extra] + 1.0])
    vr = torch.cat([data.vr, data.vr[:extra] + 1.0])
    caches = new_caches(case, data, kr, vr)
    pes = list(case.pe)
    out, live = [], []
    for st in range(case.steps):
        act = active(case, st)
        cs = [caches[i] for i in act]
        meta, new_pe = engine_cls.host_meta(stub, cs, [pes[i] for i in act])
        B = len(act)
        meta = [int(x) for x in meta]
        qkv = torch.cat([data.qkv[st, i] for i in act])
        o = launch_cpu(qkv, kr, vr, case.cap, meta[:B], meta[B:2 * B], meta[2 * B:3 * B], data.ptab, meta[3 * B:],
                       data.bu, data.bv, B, case.T, case.h, case.dk, case.scale, mut)
        engine_cls.advance(adv, cs, case.T)
        for i, p in zip(act, new_pe):
            pes[i] = p
        out.append({i: o[n * case.T:(n + 1) * case.T] for n, i in enumerate(act)})
        live.append({i: tuple(live_rows(r, c.slot, c.start, c.len, case.cap) for r in (kr, vr))
                     for i, c in zip(act, cs)})
    return out, live
