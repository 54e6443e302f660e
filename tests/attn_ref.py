"""float64 model, derived error bound and case tables of the paged attention kernels (csrc/fo_attn.hip and
csrc/fo_attn_rows.h: attn_rows_body in its k_attn_mfma instantiations, k_attn_combine, attn_arrive_and_merge,
k_attn_decode, k_attn_gqa_decode, k_attn_decode_o, on fp32, bf16 and e4m3 caches).  No GPU import:
tests/test_attn_ref_cpu.py shows on the CPU that the bound rejects wrong kernels and that every condition on the inputs
holds; tests/test_attn_exact_gpu.py launches the cases through fo.ops and fo.kv on a poisoned pool between guards.

Model.  A sequence is q [tn][H][hd], K / V [L][KVH][hd] and nvis [tn]; row (token t, head h) is softmax over the first
nvis[t] keys of kv head h // (H / KVH) of (q . K_j) scale, times V, in float64, vectorised per (sequence, kv head).  No
page, slot, item, tile or split arithmetic appears in it: that arithmetic is what is under test.  (The BOUND takes
three counts of the launch -- the tile width kt, the wave count nw, the split count ns -- and the input tables below
place keys at tile and split edges; neither feeds the model's values.)

Exact-score inputs.  scale = 2^-3 at every head size (data to the kernels; the model's own value at hd 64).  q holds
integers of -4..4, K multiples of 1/4 in -2..2, V non-zero multiples of 1/8 in -8..8.  Row (t, h) of a sequence owns the
two "structure" channels 2 r, 2 r + 1 (r = t G + h % G) of its kv head: q is 4 there (score K / 2) and 0 on every other
row's; the family of the row sets K on them.  Channels past the last row's are "free": random K, and random q on the
rand / lo_* rows only.  check_exact() proves, per row: float32(q scale) is exact; q scale, K and V split into bf16
hi + lo with zero residue; no product has two low halves (the three-product scheme drops none); every product is a
multiple of one quantum 2^-m with sum_d |q_d scale k_d| < 2^(24 - m) (the score is exact in float32 in any summation
order); s_j - max is exact.  Then the kernel's scores, maxima and exponent arguments are the model's, ties are ties,
and the bound has no score term.

Families (FAMILIES; one per row, mixed over the rows of a launch):
  flat     every visible score 0: the output is the mean of the visible V rows
  sink     key 0 at +30 over a flat rest
  own      the row's last visible key at +200: the output is that key's V row
  ends     first and last visible key at +100, middle 0: two splits weigh 1 : 1 and a middle split expf(-100), a
           subnormal number or 0 (own and descend rows give splits whose weight is 0 whatever the device expf does)
  ascend   +0.5 per key: the maximum rises in every tile
  descend  -110 - 0.5 per key: the maximum is the first key, every score far below 0
  saw      the maximum rises by 2 a tile and sits in another 16-key block (wave) each tile
  rand     random integers of -3..3 on the structure channel, random q on the free channels
  lo_q     q = 4 (1 + 2^-9) on channel 2 r against K = t_j, q = 4 on 2 r + 1 against 8 floor(j / 8) - t_j, t_j multiples
           of 8 in 0..80: the score is t_j 2^-10 + 4 floor(j / 8) -- the last 8 keys carry the row, and without the q_lo
           k_hi product their scores are equal
  lo_k     the same with the factor on K (variant "lo": not bf16-representable)
  lo_v     V = a (1 + 2^-9) on the whole kv head (variant "lo"); rand structure (ascend on a long MFMA row)
  lo_p     key 1 at the maximum with V = 0, every other key LO_P_C lower: p = expf(-LO_P_C) has a low half of
           2^-8.9 p, and without p_lo v_hi the whole row shrinks by that factor
  wide     (inexact) float q, K, V with the row's two channels at magnitude 25..40: scores of several hundred

Bound E per output element, in helper_ref's notation (U = 2^-24, gam(k) bounds k roundings, SECOND covers products of
first-order terms), EXPF = sampler_ref.EXPF for the device expf, TINY = 2^-126 where it underflows.  bf16 has 8
significant bits: |x - hi| <= 2^-8 |x|, hi + lo leaves a residue of at most RES = 2^-17 |x| (lo rounds a value
below 2^-8 |x| to 8 bits), and |lo| <= 2^-8 (1 + 2^-8) |x|.  With P_j = exp(s_j - M), w_j = P_j / sum_k P_k:

MFMA form (attn_rows_body; NT = ceil(L / kt) tiles at most, nres = NT - 1 + [ns > 1] rescales at most):
  p         expf once (EXPF); the running maximum rises at most once a tile, each rise multiplies what is held by
            alpha = expf(m_old - m_new) (EXPF, and one rounding of the accumulator: U), the merge by expf(m_q - M) once
            more: rho = (1 + EXPF)^(1 + nres) - 1 on every key's weight, numerator and denominator alike
  P . V     p = p_hi + p_lo + residue (RES p); the kernel adds p_hi v_hi + p_hi v_lo + p_lo v_hi in MFMAs of 32 products.
            No summation order or rounding mode is documented for the bf16 MFMA: any order inside one MFMA, and 2 U an
            addition.  A product that is exactly 0 adds nothing, so NPROD = 2 non-zero products a key (3 where V has a
            low half); key j's term is rounded by the additions from the start of its 32-key MFMA chunk on, and only by
            those of non-zero terms -- keys j'' below nvis with s_j'' >= s_j - 104 (a later p is taken against a maximum
            of at least s_j, and expf is 0 below -104): steps_j = NPROD #{j'' >= 32 floor(j / 32)} of those.  The merge
            adds ns products (2 U each).  nu_j = RES + 2 U steps_j + U nres + 2 U ns
            V's own residue (wide only) and the dropped p_lo v_lo: sum_j w_j (|vres_j| + 2^-8 (1 + 2^-8) |vlo_j|)
  row sum   l = l alpha + p per tile (2 roundings), row16_sum (4), the waves (nw - 1), the merge (2 ns):
            g = gam(2 NT + 4 + nw - 1 + 2 ns);  TH = sum_k w_k ((1 + rho)(1 + g) - 1)
  division  o / l, or o (1 / l) in the merge: 3 U
      E = [sum_j w_j |V_j| a_j + TH / (1 - TH) sum_j w_j |V_j| (1 + a_j) + the V terms] (1 + 3 U) + 3 U sum_j w_j |V_j|
          + 2 TINY (sum_j |V_j| + L sum_j w_j |V_j|),            a_j = (1 + rho_j)(1 + nu_j) - 1
fp32 form (attn_decode_row; kpw = 256 / hd keys a wave instruction, vstr = 8 kpw):
  scores dec_dot4 chains (exact on the exact families), one expf, the sum over ceil(L / 512) terms a thread and
  block_sum<8> (6 + 8): g = gam(ceil(L / 512) + 14); P . V a chain of ceil(L / vstr) fma a lane, log2(kpw) lane_xor
  additions, 8 wave additions: nu = gam(ceil(L / vstr) + log2(kpw) + 8); division 2 U.  No RES term.
wide only (exact=False): the score's error ds_j = A_j (2 RES + 2^-16 (1 + 2^-7) + gam(6 hd) + U), A_j = sum_d |q_d
  scale| |k_d| (two residues, the dropped low-by-low product, 3 hd products at 2 U an addition, the rounding of q
  scale; gam(hd + 1) + U on the fp32 form), and the roundings of the exponent arguments, dl_j = (1 + nres) U (M -
  min s + 2 D), D = max ds: rho_j = exp(ds_j + D + dl_j) (1 + EXPF)^(1 + nres) - 1, as relpos_ref.attend.

fo_attention_o (k_attn_decode_o): x + att Wo^T, yg = x gamma, the row's sum of squares.  The attention row's E passes
through the projection, sum_k E_k |Wo_nk|; att splits into hi + lo (RES; Wo is bf16), each head's 2 hd non-zero
products are added in MFMAs (2 U each) and the H head partials in turn: gam(4 hd + H) on sum |att| |Wo|; the residual
add, the gamma product and the stored value round once each; the squares pass ceil(D / 512) + 14 additions.

Conditions on the inputs (asserted by the CPU test, not measured): on the exact families E <= CEIL sum_j w_j |V_j| +
1e-30 (CEIL = 1e-4, the rtol of tests/test_attn_gpu.py; the 1e-30 stands for the TINY terms) on every element.  A
term that enters FIRST is rounded by all 2 NPROD L U of the additions after it, and an element may hang on its first
key alone: at NPROD 2, 4 L U + 250 U (RES, the exponentials, the row sum) <= CEIL = 1678 U needs L <= 357.  So on the
MFMA form the families that can put the weight on an early key (FRONT: sink, ends, rand) go to rows of at most
FRONT_MAXL = 330 keys, and lo_v's rand structure (NPROD 3) to at most LO_V_MAXL = 200; longer rows take the others,
whose weight sits on the last keys (own, ascend, saw, lo_q, lo_k), dies out within 208 keys (descend) or is uniform
(flat, lo_p: 2 (L + 32) U on average, within CEIL up to the tables' 643 keys).
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

from helper_ref import OBSERVED, SECOND, U, Guard, gam, gen, note, randn, ratio  # noqa: F401  (some for the tests)
from sampler_ref import EXPF

TINY = 2.0 ** -126
RES = 2.0 ** -17                         # |x - hi - lo| <= RES |x|
LOB = 2.0 ** -8 * (1 + 2.0 ** -8)        # |lo| <= LOB |x|
CEIL = 1e-4
SCALE = 2.0 ** -3
LOF = 1.0 + 2.0 ** -9                    # the lo_* operand a (1 + 2^-9): hi = a, lo = a 2^-9
LO_P_C = 1.5                             # lo_p: the common score below the maximum (p_lo = 2^-8.9 p)
FRONT = ("sink", "ends", "rand")
FRONT_MAXL = 330
LO_V_MAXL = 200
GQA_DEC_KEYS = 448                       # csrc/fo_attn.hip GQA_DEC_KEYS: k_attn_gqa_decode's single-row body up to here
EXACT_A = ("flat", "sink", "own", "ends", "ascend", "descend", "saw", "rand", "lo_q", "lo_p")
EXACT_LO = ("lo_k", "lo_v")
FAMILIES = EXACT_A + EXACT_LO + ("wide",)
O_FAMILIES = ("flat", "sink", "own", "lo_v", "rand")


def bf16_split(x):
    """float32 -> (hi, lo, residue) as float64, the kernel's split8"""
    x = x.float()
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi.double(), lo.double(), x.double() - hi.double() - lo.double()


# ------------------------------------------------------------------------------------------------ model and bound
def _steps(s, nprod):
    """s [R][L] (-inf where masked) -> steps_j [R][L] (see the docstring)"""
    L = s.shape[1]
    j = torch.arange(L)
    after = j[None, :] >= ((j // 32) * 32)[:, None]                       # [j][j'']
    live = s[:, None, :] >= (s[:, :, None] - 104.0)                       # [R][j][j'']
    return nprod * (live & after[None]).sum(-1).double()


def attend(q, K, V, nvis, H, KVH, form, kt=64, nw=4, ns=1, exact=True, scale=SCALE):
    """q [tn][H][hd] float32, K / V [L][KVH][hd] float32, nvis [tn] -> (y, E, S) [tn][H hd] float64: the model, the
    bound of the kernel form ("mfma" or "fp32") and S = sum_j w_j |V_j|."""
    tn, hd = q.shape[0], q.shape[2]
    G = H // KVH
    L = K.shape[0]
    y = torch.zeros(tn, H, hd, dtype=torch.float64)
    E, S = torch.zeros_like(y), torch.zeros_like(y)
    nv = torch.as_tensor(nvis).repeat_interleave(G)                       # [R], r = t G + g
    mask = torch.arange(L)[None, :] >= nv[:, None]
    NT = -(-L // kt)
    nres = NT - 1 + (1 if ns > 1 else 0) if form == "mfma" else 0
    for kh in range(KVH):
        Q = q[:, kh * G:(kh + 1) * G].reshape(tn * G, hd).double() * scale
        Kh, Vh = K[:, kh].double(), V[:, kh].double()
        s = (Q @ Kh.t()).masked_fill(mask, -math.inf)
        M = s.max(-1, keepdim=True).values
        w = torch.softmax(s, -1)
        aV = Vh.abs()
        _, vlo, vres = bf16_split(V[:, kh])
        if exact:
            rho = torch.full_like(s, (1 + EXPF) ** (1 + nres) - 1)
        else:
            A = Q.abs() @ Kh.abs().t()
            ds = A * ((2 * RES + 2.0 ** -16 * (1 + 2.0 ** -7) + gam(6 * hd) + U) if form == "mfma" else
                      (gam(hd + 1) + U))
            ds = ds.masked_fill(mask, 0.0)
            D = ds.max(-1, keepdim=True).values
            smin = s.masked_fill(mask, math.inf).min(-1, keepdim=True).values
            dl = (1 + nres) * U * (M - smin + 2 * D)
            rho = torch.exp(ds + D + dl) * (1 + EXPF) ** (1 + nres) - 1
        if form == "mfma":
            nprod = 3 if bool((vlo != 0).any()) else 2
            nu = RES + 2 * U * _steps(s, nprod) + U * nres + 2 * U * ns
            g = gam(2 * NT + 4 + nw - 1 + 2 * ns)
            vt = w @ (vres.abs() + LOB * vlo.abs())
            div = 3 * U
        else:
            kpw = 256 // hd
            nu = torch.full_like(s, gam(-(-L // (8 * kpw)) + int(math.log2(kpw)) + 8))
            g = gam(-(-L // 512) + 14)
            vt = torch.zeros(tn * G, hd, dtype=torch.float64)
            div = 2 * U
        a = (1 + rho) * (1 + nu) - 1
        TH = (w * ((1 + rho) * (1 + g) - 1)).sum(-1, keepdim=True)
        Sk = w @ aV
        e = ((w * a) @ aV + TH / (1 - TH) * ((w * (1 + a)) @ aV) + vt) * (1 + div) + div * Sk
        e = e * SECOND + 2 * TINY * (aV.sum(0)[None] + L * Sk)
        sl = slice(kh * G, (kh + 1) * G)
        y[:, sl] = (w @ Vh).view(tn, G, hd)
        E[:, sl] = e.view(tn, G, hd)
        S[:, sl] = Sk.view(tn, G, hd)
    return y.view(tn, H * hd), E.view(tn, H * hd), S.view(tn, H * hd)


def o_proj(x0, att, Eatt, wo, gamma, H, hd):
    """fo_attention_o after the attention: x0 [B][D] float32, att / Eatt [B][H hd] float64, wo [D][H hd] bf16, gamma
    [D] -> NS(x, Ex, yg, Eyg, ss, Ess) float64 (see the docstring)"""
    W = wo.double()
    D = W.shape[0]
    proj = att @ W.t()
    aproj = att.abs() @ W.abs().t()
    x = x0.double() + proj
    Ex = (Eatt @ W.abs().t() + (RES + gam(4 * hd + H)) * (aproj + Eatt @ W.abs().t()) + U * x.abs()) * SECOND
    g64 = gamma.double()
    yg = x * g64
    Eyg = (Ex * g64.abs() + U * yg.abs()) * SECOND
    ss = (x * x).sum(-1)
    Ess = ((2 * x.abs() * Ex + Ex * Ex).sum(-1) + gam(-(-D // 512) + 15) * ((x.abs() + Ex) ** 2).sum(-1)) * SECOND
    return NS(x=x, Ex=Ex, yg=yg, Eyg=Eyg, ss=ss, Ess=Ess)


# ------------------------------------------------------------------------------------------------ inputs
def _two(n):
    """an integer of up to 16 bits as two bf16-representable parts"""
    return n % 256, 256 * (n // 256)


def saw_hot(t, kt):
    """the saw family's raised key of tile t: another 16-key block each tile"""
    return t * kt + 16 * ((3 * t + 1) % (kt // 16)) + (5 * t) % 16


def admissible(fam, L, old, form):
    if fam in FRONT and form == "mfma":
        return L <= FRONT_MAXL
    if fam == "lo_p":
        return old >= 2            # key 1 (V = 0 there) is no token's own key
    return True


def build_seq(name, H, KVH, hd, L, tn, fams, kt, variant, form="mfma"):
    """One sequence of L keys whose last tn tokens are in the launch (causal: token i sees L - tn + 1 + i keys).  fams:
    the rotation of families, dealt to the rows (token-major) from a start that depends on the name; a family that
    is not admissible at this length is passed over.  -> NS(q, K, V, nvis, fam [tn][H])"""
    G = H // KVH
    R = tn * G
    assert 1 <= tn <= L and 2 * R <= hd, name
    g = gen("attn/" + name)
    old = L - tn
    nvis = [old + 1 + i for i in range(tn)]
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()   # noqa: E731
    if variant == "wide":
        q, K, V = randn(g, tn, H, hd), randn(g, L, KVH, hd), randn(g, L, KVH, hd) * 2.0
        sg = lambda *shape: ri(0, 1, *shape) * 2 - 1                                     # noqa: E731
        mag = lambda *shape: (25 + 15 * torch.rand(*shape, generator=g)) * sg(*shape)    # noqa: E731
        for i in range(tn):
            for h in range(H):
                c = 2 * (i * G + h % G)
                q[i, h, c:c + 2] = mag(2)
                K[:, h // G, c:c + 2] = mag(L, 2)
        return NS(q=q, K=K, V=V, nvis=nvis, fam=[["wide"] * H for _ in range(tn)])
    q = torch.zeros(tn, H, hd)
    K = ri(-8, 8, L, KVH, hd) / 4
    K[:, :, :2 * R] = 0.0
    V = ri(1, 64, L, KVH, hd) / 8 * (ri(0, 1, L, KVH, hd) * 2 - 1)
    if variant == "lo":
        V = V * LOF
    if old >= 2:
        V[1] = 0.0
    fam = [[None] * H for _ in range(tn)]
    at = int(torch.randint(0, len(fams), (1,), generator=g))
    free = slice(2 * R, hd)
    for i in range(tn):
        for h in range(H):
            kh, c = h // G, 2 * (i * G + h % G)
            while not admissible(fams[at % len(fams)], L, old, form):
                at += 1
            f = fams[at % len(fams)]
            at += 1
            if "own" in fams and h == 0 and nvis[i] % kt == 0:
                f = "own"                                 # its own key is the last of a tile
            fam[i][h] = f
            nv = nvis[i]
            q[i, h, c] = q[i, h, c + 1] = 4.0
            col = K[:, kh, c:c + 2]                       # (a view)
            if f == "sink":
                col[0, 0] = 60.0
            elif f == "own":
                col[nv - 1, 0] = 400.0
            elif f == "ends":
                col[0, 0] = col[nv - 1, 0] = 200.0
            elif f in ("ascend", "descend") or (f == "lo_v" and form == "mfma" and L > LO_V_MAXL):
                a, b = _two(torch.arange(L) + (220 if f == "descend" else 0))
                sg = -1.0 if f == "descend" else 1.0
                col[:, 0], col[:, 1] = sg * a.float(), sg * b.float()
            elif f == "saw":
                for t in range(-(-L // kt)):
                    if saw_hot(t, kt) < L:
                        col[saw_hot(t, kt), 0] = 4.0 * (t + 1)
            elif f in ("rand", "lo_v"):
                col[:, 0] = ri(-6, 6, L)
                q[i, h, free] = ri(-4, 4, hd - 2 * R)
            elif f in ("lo_q", "lo_k"):
                t_ = ri(0, 10, L) * 8
                t_[nv - 1] = 80.0
                t_[max(0, nv - 2)] = 0.0
                col[:, 0], col[:, 1] = t_ * (LOF if f == "lo_k" else 1.0), 8.0 * (torch.arange(L) // 8) - t_
                q[i, h, c] = 4.0 * (LOF if f == "lo_q" else 1.0)
                q[i, h, free] = ri(-4, 4, hd - 2 * R)
            elif f == "lo_p":
                col[:, 0] = -2 * LO_P_C
                col[1, 0] = 0.0
            else:
                assert f == "flat", f
    return NS(q=q, K=K, V=V, nvis=nvis, fam=fam)


def check_exact(sq, H, KVH):
    """The exactness properties of the docstring for every row of a sequence built from the exact families."""
    G = H // KVH
    qs = sq.q.double() * SCALE
    assert torch.equal(qs, (sq.q * np.float32(SCALE)).double()), "float32(q scale) is not exact"
    qh, ql, qr = bf16_split(sq.q * np.float32(SCALE))
    kh_, kl, kr = bf16_split(sq.K)
    _, _, vr = bf16_split(sq.V)
    assert not qr.any() and not kr.any() and not vr.any(), "a bf16 hi + lo split leaves a residue"
    for i, nv in enumerate(sq.nvis):
        for h in range(H):
            kh = h // G
            assert not (ql[i, h].abs()[None] * kl[:nv, kh].abs()).any(), "a product of two low halves"
            prod = qs[i, h][None] * sq.K[:nv, kh].double()                 # [nv][hd], exact in float64
            nz = prod[prod != 0]
            if not nz.numel():
                continue
            m = 0
            while bool((torch.round(nz * 2.0 ** m) != nz * 2.0 ** m).any()):
                m += 1
                assert m < 24
            assert float(prod.abs().sum(-1).max()) < 2.0 ** (24 - m), (sq.fam[i][h], m)
            s = prod.sum(-1)
            d = s - s.max()
            assert torch.equal(d.float().double(), d) and torch.equal(s.float().double(), s), "s - max rounds"


# ------------------------------------------------------------------------------------------------ case tables
def split_count(Lmax, nsplit, kps):
    """splits an item of Lmax keys takes (attn_rows_body): nsplit static, or by tickets min(nsplit, ceil(Lmax / kps))"""
    return nsplit if not kps else min(nsplit, max(1, -(-Lmax // kps)))


def split_len(Lmax, ns, kt):
    return -(-(-(-Lmax // ns)) // kt) * kt


def _case(name, H, KVH, hd, kt, nw, seqs, variant="A", form="mfma", rows=16, splits=((1, 0),)):
    """seqs: [(L, tn)]; splits: [(nsplit, keys per split; 0: static splits + k_attn_combine)]"""
    fams = {"A": EXACT_A, "lo": EXACT_LO, "wide": ("wide",), "o": O_FAMILIES}[variant]

    def build():
        return [build_seq(f"{name}/{si}", H, KVH, hd, L, tn, fams, kt, "lo" if variant == "o" else variant,
                          "fp32" if form == "fp32" or (form == "gqa" and L <= GQA_DEC_KEYS) else "mfma")
                for si, (L, tn) in enumerate(seqs)]
    return NS(name=f"{name}/{variant}", H=H, KVH=KVH, hd=hd, kt=kt, nw=nw, seqs=seqs, variant=variant, form=form,
              rows=rows, tpi=max(1, rows // (H // KVH)), splits=splits, exact=variant != "wide", bf16=variant == "A",
              build=build)


def seq_form(case, L):
    """the body an item of L keys takes: k_attn_gqa_decode chooses per item"""
    if case.form == "gqa":
        return "fp32" if L <= GQA_DEC_KEYS else "mfma"
    return case.form


def reference(case, data, ns):
    """-> per sequence (y, E, S) for a launch with ns split slots"""
    return [attend(sq.q, sq.K, sq.V, sq.nvis, case.H, case.KVH, seq_form(case, L), case.kt, case.nw, ns, case.exact)
            for sq, (L, _) in zip(data, case.seqs)]


def _ladder(kt, tns):
    return list(zip([1, 2, kt - 1, kt, kt + 1, 2 * kt + 1, 5 * kt + 3], tns))


ROWS4 = [(1, 0), (3, 0), (4, 64)]                    # one split; static splits + combine; tickets
TN8 = [1, 2, 8, 3, 2, 8, 5]
DEC_L = [1, 15, 16, 17, 223, 224, 225, 511, 512, 513, 1025]       # 224: the end of hd 128's 14 prefetch rounds
VARIANTS = ("A", "lo", "wide")
MFMA_CASES = [c for v in VARIANTS for c in (
    _case("mfma32", 4, 2, 32, 64, 4, _ladder(64, TN8), v, splits=ROWS4),
    _case("mfma64", 4, 2, 64, 64, 4, _ladder(64, TN8), v, splits=ROWS4),
    _case("mfma128x8", 14, 2, 128, 128, 8, _ladder(128, [1, 2, 2, 2, 2, 2, 2]), v,
          splits=[(1, 0), (3, 0), (4, 128), (4, 256)]),
    _case("mfma128x8x2", 14, 2, 128, 128, 8, [(127, 4), (129, 4), (386, 4)], v, rows=32, splits=[(1, 0), (4, 128)]),
    _case("mfma128x2", 14, 2, 128, 32, 2, [(1, 1), (31, 2), (32, 2), (33, 2), (97, 2)], v, splits=[(4, 32)]),
)]
GQA_CASES = [_case("gqa128", 14, 2, 128, 128, 8, [(L, 1) for L in (1, 447, 448, 449, 600)], v, form="gqa",
                   splits=[(1, 0), (4, 128)]) for v in VARIANTS]
DECODE_CASES = [_case(f"decode{hd}", 4, 4, hd, 64, 8, [(L, 1) for L in DEC_L], v, form="fp32")
                for hd in (32, 64, 128) for v in VARIANTS]
O_CASE = _case("decode_o64", 14, 14, 64, 64, 8, [(1, 1), (17, 1), (513, 1), (64, 1)], "o", form="fp32")
GROUP = NS(B=4, To=2, C=4, H=14, KVH=2, hd=128, kt=128, nw=8, olds=[15, 1, 37, 123], nsplit=4, kps=128)
GROUP_CASES = [_case("group128", GROUP.H, GROUP.KVH, GROUP.hd, GROUP.kt, GROUP.nw,
                     [(n + GROUP.C * GROUP.To, GROUP.C * GROUP.To) for n in GROUP.olds], v,
                     splits=[(GROUP.nsplit, GROUP.kps)]) for v in ("A", "lo")]
for _c in GROUP_CASES:
    _c.tpi = GROUP.To
ALL_CASES = MFMA_CASES + GQA_CASES + DECODE_CASES + GROUP_CASES + [O_CASE]


def o_inputs(case):
    """fo_attention_o's other operands: Wo bf16 [D][H hd] from a small dyadic set, gamma, the residual rows"""
    g = gen("attn/o/" + case.name)
    D, K = 896, case.H * case.hd
    wo = (torch.randint(-4, 5, (D, K), generator=g).float() / 64).bfloat16()
    return NS(D=D, wo=wo, gamma=1 + 0.1 * randn(g, D), x0=randn(g, len(case.seqs), D))
