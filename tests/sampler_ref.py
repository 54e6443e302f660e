"""float64 model of the token sampler (csrc/fo_sample.hip), the case tables the CPU and GPU tests share, and the
acceptance rules that compare a kernel's output with the model.

The model follows the documented rule (models/audioLLM.py:431-477, models/decoder/decoder.py:348-359, and the header
and comments of fo_sample.hip), not the kernel's control flow: it sorts where the kernel selects by radix, and it sums
in float64.

The rule
  * A banned id (0 <= ban < V) is removed before anything else.
  * top-k applies when 0 < k < allowed count; ties at the threshold go to the smaller index.
  * top-p (p > 0) keeps the longest prefix, in descending value, whose inclusive cumulative probability (of the top-k
    renormalised distribution) is <= p; the first token alone when even that exceeds p.
  * Two code paths, and the two documented deviations the tests pin as they are (DESIGN "Sampling RNG"):
      - "general" (k == 0, k > 64 or k >= allowed): a group of equal logits at the top-p boundary is kept whole or
        dropped whole; when the top group itself does not fit, only its smallest index is kept.  "Equal" is equality
        of the order-preserving integer key, under which -0.0 sorts below +0.0.  The CDF of the draw runs in index
        order.
      - "small" (1 <= k <= 64 and k < allowed): tokens are taken one by one in (value descending, index ascending)
        order, so a tie group can be cut; -0.0 == +0.0 here (a float comparison).  The CDF runs in that sorted order.
    The reference (torch.sort + cumsum) takes tied tokens one by one in an order it does not specify, so neither
    path can be "the" reference on a tie; the tests hold each path to its own documented rule.
  * The draw: u = u01(seed, key, step); the id whose CDF interval holds u.

Exponent.  To keep the bound tight the model forms the exponent as the kernel does, in float32 -- float32(x - m) *
float32(1 / T) on the general path, float32(x - m) / float32(T) on the small path (both IEEE operations on the device)
-- and then takes exp in float64.  What is left between model and kernel is the device expf and the float32 sums.

Tolerance delta(path, V, k) (derived, not tuned).  It bounds, in units of the normaliser Z, the error of any prefix sum
of kept masses the kernel compares with, plus the error of its target u * Z.  Every partial sum is <= Z, so one float32
operation on it costs at most EPS = 2^-24 (in units of Z); every mass carries the device expf's relative error EXPF.
  general, C = ceil(V / 1024) tokens per thread:
      prefix = wave totals before (<= 16 adds) + wave scan (6) + own run (C) + "base + inc - v" (2) + walk (<= C)
      Z      = own run (C) + wave scan (6) + 16 wave totals
      target = 1 multiply
      => (3 C + 47) EPS, written as (3 C + 48) EPS
  small, at most 64 candidates:
      z = k sequential adds, prefix = <= k adds, target = 1 multiply (the distribution: one division more)
      => (2 k + 2) EPS
  both: + 2 EXPF, one for the prefix and one for Z.  EXPF = 2^-22: the device library documents expf at 1 ulp
  (2^-23 relative); one more is allowed for the documented figure being a tested maximum, not a proof.

Acceptance of a draw.  Id i passes iff it is kept and u lies in [cdf_lo(i) - delta, cdf_hi(i) + delta] of the float64
CDF in the path's order.  No draw is skipped.  A u within delta of an interior edge lets two ids pass; the share of such
draws is a condition on the table (<= 5 % per case, from the model alone), which is why the draw cases keep the kept
set at a few thousand tokens.

Acceptance of a distribution (fo_sample_probs).  The support must equal the model's exactly; values within delta
relative, with a floor of 2^-32 absolute (the top-p pass works in 32.32 fixed point and cannot see less).  "Support":
a kept token whose mass is zero (a -inf logit inside the top k) is written as 0 by the kernel, and a mass below the
smallest normal float32 may flush to 0, so such tokens are compared by value only.

top-p values come from the model per row: the float32 midpoint of two adjacent cumulative masses whose neighbouring
token (small) or group (general) weighs >= 64 delta on either side of p, so the model alone decides the kept set
(the kernel's own top-p arithmetic -- k float32 divisions and adds, or V truncations of 2^-32 -- stays far inside).
One case sits exactly on a cumulative value; all its masses are 1.0 and the arithmetic is exact in every format.
"""
import zlib
from types import SimpleNamespace as NS

import numpy as np

M64 = (1 << 64) - 1
EPS = 2.0 ** -24
EXPF = 2.0 ** -22
KMAXS = 64          # largest k of the small path
NSTREAM = 512       # streams per draw case
FLOOR = 2.0 ** -32
TINY = 2.0 ** -126  # smallest normal float32
MARGIN = 64         # top-p margin in units of delta
AMBIG_MAX = 0.05

DRAW_MUTANTS = ("row_key", "no_step", "prec", "order_general", "order_small", "shift", "ban_k", "no_T_general",
                "no_T_small")
SET_MUTANTS = ("topk_tie_last", "split_general", "whole_small", "ban_norm", "topp_lt")


# ------------------------------------------------------------------------------------------------ the stream
def smix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u01(seed, key, step, mut=None):
    """The kernel's counter stream, exact: splitmix64 of seed ^ ((0x9E37 * (key + 1)) + step) -- '+' binds before '^'
    in C -- top 24 bits / 2^24.  mut "prec": the other precedence."""
    seed, key, step = int(seed) & M64, int(key), int(step)
    a = (0x9E37 * (key + 1)) & M64
    x = ((seed ^ a) + step) & M64 if mut == "prec" else seed ^ ((a + step) & M64)
    return (smix(x) >> 40) / 16777216.0


def delta(path, V, k):
    if path == "small":
        return (2 * min(max(k, 1), KMAXS) + 2) * EPS + 2 * EXPF
    C = -(-V // 1024)
    return (3 * C + 48) * EPS + 2 * EXPF


def path_of(V, k, ban):
    allowed = V - (1 if 0 <= ban < V else 0)
    return "small" if 1 <= k <= KMAXS and k < allowed else "general"


def fkey(x):
    """order-preserving float32 -> integer key (larger float, larger key; -0.0 below +0.0)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u >> 31, (~u) & 0xFFFFFFFF, u | 0x80000000)


def _leading(ok):
    return int(len(ok) if ok.all() else np.argmin(ok))


# ------------------------------------------------------------------------------------------------ the model
def model(lg, k, T, p, ban=-1, mut=()):
    """The kept set and its distribution.  Returns a namespace: path, delta, kept [V] bool, prob [V] float64, order
    (kept ids in the CDF's order), lo / hi [V] (CDF interval of every kept id), margin (distance of p to the nearest
    cumulative value that would change the set; inf without top-p), and the top-k stage (sel, e, gkey) for the table
    builder.  mut: names of deliberate faults (tests/test_sampler_ref_cpu.py)."""
    lg = np.asarray(lg, np.float32)
    V = lg.size
    k = int(k)
    T32 = np.float32(T)
    p = float(np.float32(p))
    allowed = np.ones(V, bool)
    if 0 <= ban < V:
        allowed[ban] = False
    ncmp = V if "ban_k" in mut else int(allowed.sum())
    small = 1 <= k <= KMAXS and k < ncmp
    path = "small" if small else "general"
    key = fkey(lg + np.float32(0.0)) if small else fkey(lg)      # x + 0.0 turns -0.0 into +0.0
    cand = np.flatnonzero(allowed)
    tie = -cand if "topk_tie_last" in mut else cand
    o = cand[np.lexsort((tie, -key[cand]))]
    sel = o[:k] if 0 < k < ncmp else o
    sel = sel[np.lexsort((sel, -key[sel]))]
    m = lg[sel[0]]
    with np.errstate(invalid="ignore"):
        d = (lg[sel] - m).astype(np.float32)
        if small:
            a = d if "no_T_small" in mut else (d / T32).astype(np.float32)
        else:
            a = d if "no_T_general" in mut else (d * (np.float32(1.0) / T32)).astype(np.float32)
    e = np.exp(a.astype(np.float64))
    Z = e.sum()
    if "ban_norm" in mut and 0 <= ban < V:
        with np.errstate(invalid="ignore", over="ignore"):
            Z = Z + float(np.exp(np.float64(np.float32(np.float32(lg[ban] - m) / T32))))
    n = len(sel)
    keep, margin = n, np.inf
    gkey = key[sel]
    if p > 0 and n > 1:
        cum = np.cumsum(e) / Z
        grouped = ("whole_small" in mut) if small else ("split_general" not in mut)
        ends = np.flatnonzero(np.append(gkey[1:] != gkey[:-1], True)) if grouped else np.arange(n)
        U = cum[ends]
        ok = (U < p) if "topp_lt" in mut else (U <= p)
        nfit = _leading(ok)
        keep = int(ends[nfit - 1]) + 1 if nfit else 1
        below = U[nfit - 1] if nfit else 0.0
        above = U[nfit] if nfit < len(U) else np.inf
        margin = min(p - below, above - p)
    ids = sel[:keep]
    kept = np.zeros(V, bool)
    kept[ids] = True
    prob = np.zeros(V)
    prob[ids] = e[:keep] / e[:keep].sum()
    in_index_order = small if "order_small" in mut else (not small and "order_general" not in mut)
    order = np.sort(ids) if in_index_order else ids
    chi = np.cumsum(prob[order])
    clo = chi - prob[order]
    chi[-1] = 1.0
    lo, hi = np.full(V, np.nan), np.full(V, np.nan)
    lo[order], hi[order] = clo, chi
    return NS(path=path, delta=delta(path, V, k), kept=kept, prob=prob, order=order, chi=chi, lo=lo, hi=hi,
              margin=margin, sel=sel, e=e, Z=Z, gkey=gkey, V=V, k=k, p=p)


def kept_set(logits, k, T, p, ban=-1):
    """(kept mask, float64 probabilities, order of the CDF)"""
    r = model(logits, k, T, p, ban)
    return r.kept, r.prob, r.order


def pick(mod, u, mut=()):
    """The id the rule draws at u: the first id in CDF order with u < cdf_hi.  mut "shift": the next kept one."""
    j = min(int(np.searchsorted(mod.chi, u, side="right")), len(mod.order) - 1)
    if "shift" in mut:
        j = min(j + 1, len(mod.order) - 1)
    return int(mod.order[j])


def excess(mod, i, u):
    """How far u lies outside id i's CDF interval, in units of delta (inf: i is not kept or not an id)."""
    if not (0 <= i < mod.V) or not mod.kept[i]:
        return np.inf
    return max(mod.lo[i] - u, u - mod.hi[i], 0.0) / mod.delta


def accepted(mod, i, u):
    return excess(mod, i, u) <= 1.0


def edges(mod):
    e = np.unique(mod.chi[:-1])
    return e[(e > 0) & (e < 1)]


def ambiguous_share(mod, us):
    """(observed, predicted) share of draws within delta of an interior CDF edge, where two ids pass."""
    e = edges(mod)
    if not len(e):
        return 0.0, 0.0
    us = np.asarray(us)
    j = np.clip(np.searchsorted(e, us), 1, len(e) - 1) if len(e) > 1 else np.zeros(len(us), int)
    dist = np.minimum(np.abs(us - e[j]), np.abs(us - e[j - 1])) if len(e) > 1 else np.abs(us - e[0])
    return float(np.mean(dist <= mod.delta)), min(1.0, 2 * mod.delta * len(e))


def probs_error(mod, got):
    """Compare a row of fo_sample_probs with the model.  Returns (support_ok, max error / bound) with bound =
    max(delta * prob, 2^-32)."""
    got = np.asarray(got, np.float64)
    solid = mod.kept & (mod.prob >= TINY)
    support_ok = bool(np.all(got[solid] > 0) and np.all(got[~mod.kept] == 0))
    bound = np.maximum(mod.delta * mod.prob, FLOOR)
    return support_ok, float(np.max(np.abs(got - mod.prob) / bound))


# ------------------------------------------------------------------------------------------------ rows
VS = (5, 64, 65, 1000, 1025, 4096, 5000)
FAMS = ("wide", "narrow", "quant", "zeros", "inf3", "inf40", "const")
TIE_FREE = ("wide", "narrow")
TS = (0.25, 0.7, 1.0, 1.6)
BANS = ("none", "argmax", "intopk", "tie", "beyond")
_ROWS = {}


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_row(fam, V):
    """One logits row of a family, deterministic in (fam, V)."""
    if (fam, V) in _ROWS:
        return _ROWS[fam, V]
    rng = rng_of(f"row/{fam}/{V}")
    g = rng.standard_normal(V).astype(np.float32)
    if fam == "wide":
        r = g * np.float32(3.0)
    elif fam == "narrow":
        r = g * np.float32(0.7)
    elif fam == "quant":                      # many ties, ties at the maximum
        r = np.round(g * 2) / 2
        r[rng.integers(0, V, 2)] = r.max()
    elif fam == "zeros":                      # -0.0 against +0.0, below a unique maximum
        r = np.round(g * 2) / 2
        z = r == 0
        r[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
        r[0], r[1], r[V - 1] = -0.0, 0.0, max(float(r.max()), 0.0) + 0.5
    elif fam == "inf3":                       # all but 3 entries -inf
        r = np.full(V, -np.inf, np.float32)
        r[rng.permutation(V)[:3]] = np.float32([0.75, -0.5, 1.5])
    elif fam == "inf40":                      # 40 % -inf
        r = g * np.float32(3.0)
        r[rng.permutation(V)[:(2 * V) // 5]] = -np.inf
    elif fam == "const":
        r = np.full(V, 1.25, np.float32)
    elif fam == "fin64":                      # tie-free, exactly 64 finite logits (the k = 64 against 65 pair)
        r = np.full(V, -np.inf, np.float32)
        r[rng.permutation(V)[:64]] = (rng.permutation(64) * 0.11 - 3.0).astype(np.float32)
    elif fam == "dyadic":                     # four equal finite logits: every mass is exactly 1
        r = np.full(V, -np.inf, np.float32)
        r[rng.permutation(V)[:4]] = 2.0
    else:
        raise KeyError(fam)
    r = np.ascontiguousarray(r, np.float32)
    r.setflags(write=False)
    _ROWS[fam, V] = r
    return r


def ban_id(row, kind):
    """The banned id of a ban variant: the arg-max, a token inside the top k, a token on the k = 5 tie threshold,
    an id >= V (ignored), or none."""
    V = row.size
    o = np.lexsort((np.arange(V), -fkey(row + np.float32(0.0))))
    if kind == "none":
        return -1
    if kind == "argmax":
        return int(o[0])
    if kind == "intopk":
        return int(o[min(2, V - 1)])
    if kind == "tie":
        t = row[o[min(4, V - 1)]]
        return int(np.flatnonzero(row == t)[0])
    if kind == "beyond":
        return V + 3
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------------ top-p values
def _f32(x):
    return float(np.float32(x))


def topp_value(row, k, T, ban, kind):
    """A top-p value of the given kind for (row, k, T, ban), or None when the row has no boundary with the margin.
      mid    midpoint of two adjacent cumulative masses (units: tokens on the small path, tie groups on the general),
             the boundary nearest 0.7 whose margin holds
      first  below the first unit's mass (the "first only" shift)
      tie    midpoint of two token-level cumulative masses inside one group of equal logits
      exact  exactly the cumulative mass of the first half of the tokens (dyadic rows only)"""
    b = model(row, k, T, 0.0, ban)
    n = len(b.sel)
    if n < 2:
        return None
    cum = np.cumsum(b.e) / b.Z
    need = MARGIN * b.delta

    def holds(p):
        return p is not None and 0 < p < 1 and model(row, k, T, p, ban).margin >= need

    if kind == "exact":
        return _f32(cum[n // 2 - 1])
    if kind == "first":
        grouped = b.path == "general"
        first = cum[np.flatnonzero(np.append(b.gkey[1:] != b.gkey[:-1], True))[0]] if grouped else cum[0]
        p = _f32(first / 2)
        return p if holds(p) else None
    if kind == "mid":
        ends = np.flatnonzero(np.append(b.gkey[1:] != b.gkey[:-1], True)) if b.path == "general" else np.arange(n)
        U = cum[ends]
        for j in np.argsort(np.abs(U[:-1] - 0.7), kind="stable")[:8]:
            p = _f32((U[j] + U[j + 1]) / 2)
            if holds(p):
                return p
        return None
    if kind == "tie":
        inside = np.flatnonzero(b.gkey[1:] == b.gkey[:-1])          # j and j + 1 in one group
        for j in inside[np.argsort(np.abs(cum[inside] - 0.6), kind="stable")][:8]:
            p = _f32((cum[j] + cum[j + 1]) / 2)
            if holds(p):
                return p
        return None
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------------ distribution table
def ks_of(V):
    return sorted({k for k in (0, 1, 2, 5, 63, 64, 65, 100, V - 1, V, V + 7)})


_GROUPS = None


def dist_groups():
    """The distribution table: one group per (V, family, ban variant) = one launch over a shared row (ld == 0) whose
    rows carry their own (k, T, p) and so take different paths in one grid.  Each setting: (k, T, p, p kind, path)."""
    global _GROUPS
    if _GROUPS is not None:
        return _GROUPS
    out = []
    for vi, V in enumerate(VS):
        for fi, fam in enumerate(FAMS):
            row = make_row(fam, V)
            for bi, bk in enumerate(BANS):
                if V >= 4096 and bk != "none" and (bi + fi + vi) % 2:     # half of the ban variants at the large V
                    continue
                ban = ban_id(row, bk)
                st = []
                for ki, k in enumerate(ks_of(V)):
                    T = TS[(ki + fi + vi) % 4]
                    kinds = ["none"] if k == 1 else ["none", "mid", ("first", "tie", "mid")[ki % 3]]
                    for kind in dict.fromkeys(kinds):
                        p = 0.0 if kind == "none" else topp_value(row, k, T, ban, kind)
                        if p is not None:
                            st.append((k, T, p, kind, path_of(V, k, ban)))
                out.append(NS(name=f"{fam}/V{V}/ban-{bk}", V=V, fam=fam, row=row, ban=ban, bank=bk, settings=st))
    # the k = 64 against 65 pair on a tie-free row with exactly 64 finite logits: the same support on both paths
    for V in (65, 1000, 4096):
        row = make_row("fin64", V)
        st = []
        for T in (0.7, 1.6):
            for kind in ("none", "mid", "first"):
                p = 0.0 if kind == "none" else topp_value(row, 64, T, -1, kind)
                if p is not None:
                    st += [(64, T, p, kind, "small"), (65, T, p, kind, "general")]
        out.append(NS(name=f"fin64/V{V}/ban-none", V=V, fam="fin64", row=row, ban=-1, bank="none", settings=st))
    # a boundary exactly on a cumulative value (every mass is 1.0: exact in float32, float64 and 32.32 fixed point)
    row = make_row("dyadic", 64)
    out.append(NS(name="dyadic/V64/ban-none", V=64, fam="dyadic", row=row, ban=-1, bank="none",
                  settings=[(4, 1.0, topp_value(row, 4, 1.0, -1, "exact"), "exact", "small")]))
    _GROUPS = out
    return out


# ------------------------------------------------------------------------------------------------ draw table
def streams(name, n=NSTREAM):
    """seed, keys (distinct, with gaps, in no order) and steps of the n streams of a draw case"""
    rng = rng_of("streams/" + name)
    seed = (int(rng.integers(0, 2 ** 62)) << 2) | 1
    return seed, rng.permutation(4 * n)[:n].astype(np.int32), rng.integers(0, 100000, n).astype(np.int32)


def stream_us(seed, keys, steps, mut=()):
    return np.array([u01(seed, r if "row_key" in mut else keys[r], 0 if "no_step" in mut else steps[r],
                         "prec" if "prec" in mut else None) for r in range(len(keys))])


_DRAWS = None


def draw_cases():
    """(name, family, V, k, T, p kind, ban kind, path): each run as NSTREAM streams of one shared row."""
    global _DRAWS
    if _DRAWS is not None:
        return _DRAWS
    spec = [
        ("full-4096", "wide", 4096, 0, 1.0, "none", "none"),          # 4 tokens per thread: picks at run boundaries
        ("full-5000-p", "wide", 5000, 0, 0.7, "mid", "none"),
        ("flat-1025", "narrow", 1025, 0, 1.6, "none", "argmax"),      # flat: streams differ, a wrong key shows
        ("k100-quant", "quant", 1025, 100, 1.0, "none", "none"),      # top-k ties taken in index order
        ("k200-narrow", "narrow", 4096, 200, 1.6, "none", "intopk"),
        ("group-p-quant", "quant", 1000, 0, 1.0, "tie", "none"),      # a top-p boundary inside a tie group
        ("first-only", "wide", 1000, 0, 0.25, "first", "none"),
        ("inf40-cold", "inf40", 1025, 0, 0.25, "none", "none"),
        ("k-eq-allowed", "narrow", 65, 64, 1.0, "none", "intopk"),    # k == allowed count: general, not small
        ("k5-wide", "wide", 1000, 5, 0.7, "none", "none"),
        ("k64-narrow", "narrow", 4096, 64, 1.6, "none", "tie"),
        ("k63-quant-p", "quant", 65, 63, 1.0, "tie", "none"),         # a tie group cut one by one
        ("k2-tiny", "wide", 5, 2, 1.0, "none", "none"),
        ("k5-inf3", "inf3", 64, 5, 1.0, "none", "none"),              # k above the number of finite logits
        ("k20-zeros-p", "zeros", 1000, 20, 1.6, "mid", "argmax"),
    ]
    out = []
    for name, fam, V, k, T, pk, bk in spec:
        row = make_row(fam, V)
        ban = ban_id(row, bk)
        p = 0.0 if pk == "none" else topp_value(row, k, T, ban, pk)
        assert p is not None, name
        seed, keys, steps = streams(name)
        out.append(NS(name=name, fam=fam, V=V, row=row, k=k, T=T, p=p, ban=ban, path=path_of(V, k, ban), seed=seed,
                      keys=keys, steps=steps))
    _DRAWS = out
    return out
