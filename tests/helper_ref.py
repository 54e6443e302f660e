"""float64 models, derived error bounds and case tables of the small kernels around the large ones:
csrc/fo_elem.hip (rmsnorm, layernorm, gather_rows, im2col_conv1d, conv_cache_update, scale, fill_hash), fo_fbank
(csrc/fo_audio.hip), the silence cut (k_silence_cut, csrc/fo_codec.hip) and the codec encoder's kernels
(csrc/fo_codec_enc.hip: conv1d_ex, group_norm, gte_head, vq_nearest).  No GPU import: tests/test_helper_ref_cpu.py
shows on the CPU that the bounds reject wrong kernels and that every condition on the inputs holds; the GPU tests
(test_helper_kernels_gpu.py, test_codec_enc_kernels_gpu.py) launch the cases through fo.ops between guards.

Notation.  U = 2^-24, one float32 rounding (half an ulp, relative).  gam(k) = k U / (1 - k U) bounds k roundings in a
chain.  A block-wide sum (fo_common.h block_sum<4>) adds, after each thread's own n_t terms, 6 butterfly levels and
the 4 wave sums: a term passes through at most n_t + 10 additions, so |sum_k - sum| <= gam(n_t + 10) sum |terms|
(+ 1 where the term itself is a rounded product).  IEEE operations (+, *, fma, and / and sqrtf, which hipcc rounds
correctly by default) cost U each; a division is counted as 2 U all the same.

Device math library.  ROCm ships no accuracy table for rsqrtf, erff and logf on this installation, so each was measured
alone against the host's double function (tests/mathlib_probe.hip, 2^22 log-spaced points) on an MI355X:
    rsqrtf on [1e-12, 1e8]               worst 0.853 ulp
    erff   on +-[1e-6, 6]                worst 1.501 ulp
    logf   on [1e-8, 1e16]               worst 2.316 ulp
    (sqrtf and 1/x on [1e-12, 1e8]: 0.5 ulp each, correctly rounded)
The bounds use TWICE the observed figure, as a relative error of ulps * 2^-23 (an ulp is at most 2^-23 relative).
None of these figures comes from a kernel under test.

Exact operations (gather_rows with its bf16 table and fp16 rounding, im2col_conv1d, conv_cache_update, scale,
fill_hash, the VQ residual, the silence cut on dyadic rows) have no bound: their tests use torch.equal.
"""
import math
import zlib
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

from oracle import weights as ow

U = 2.0 ** -24
RSQRT_OBS, ERF_OBS, LOG_OBS = 0.853, 1.501, 2.316    # observed worst ulps (see the docstring)
RSQRT_REL, ERF_REL, LOG_REL = (2 * v * 2.0 ** -23 for v in (RSQRT_OBS, ERF_OBS, LOG_OBS))
SECOND = 1.0 + 2.0 ** -20                              # covers the products of first-order terms
SENT = 12345.678
ISENT = -77777
SLOPE32 = float(np.float32(0.1))
THIRD = float(np.float32(1.0 / 3.0))
FLT_EPS = float(np.float32(1.1920928955078125e-07))


def gam(k):
    return k * U / (1.0 - k * U)


def inv_sqrt_rel(rho):
    """relative error of q^-1/2 when q carries the relative error rho: (1 - rho)^-1/2 <= 1 + (rho / 2) / (1 - rho)"""
    return 0.5 * rho / (1.0 - rho)


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def f16_of_f64(a):
    """float64 -> nearest fp16 value, one rounding (numpy converts directly, not through float32)"""
    return torch.from_numpy(a.numpy().astype(np.float16).astype(np.float64))


OBSERVED = {}


def note(family, r):
    OBSERVED[family] = max(OBSERVED.get(family, 0.0), r)
    return r


def ratio(got, y, E):
    """max |got - y| / E over the elements (0 where they agree exactly); non-finite outputs fail"""
    err = (got.double() - y).abs()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(torch.where(err == 0, torch.zeros_like(err), err / E).max()) if err.numel() else 0.0


class Guard:
    """A device tensor of `shape` inside a sentinel-filled allocation (64 guard elements either side: the view stays
    16-byte aligned).  mask: what a launch may write.  check(): every other byte came back bit-identical."""
    PAD = 64

    def __init__(self, dev, *shape, dtype=torch.float32, fill=None):
        n = int(np.prod(shape)) if shape else 1
        fill = (SENT if dtype.is_floating_point else ISENT) if fill is None else fill
        self.full = torch.full((2 * self.PAD + n,), fill, dtype=dtype, device=dev)
        self.t = self.full[self.PAD:self.PAD + n].view(*shape)
        self.mask = torch.zeros(*shape, dtype=torch.bool)
        self.init = None

    def arm(self):
        self.init = self.full.cpu().clone()
        return self

    @staticmethod
    def _bits(t):
        return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])

    def check(self, what):
        got = self.full.cpu()
        keep = torch.ones(got.shape, dtype=torch.bool)
        keep[self.PAD:got.numel() - self.PAD] = ~self.mask.reshape(-1)
        assert torch.equal(self._bits(got)[keep], self._bits(self.init)[keep]), \
            f"{what}: a guard element or a position the launch may not write changed"
        return got[self.PAD:got.numel() - self.PAD].view(self.mask.shape)


# ================================================================================================ A. fo_elem.hip
# ------------------------------------------------------------------------------------------------ rmsnorm
# k_rmsnorm: s = block_sum of x^2 (each thread 4 products and 4 additions per pass of 1024 columns), r = rsqrtf(s / D
# + eps), out = g * (x * r), x * r rounded to fp16 first when round_fp16.
RMS_EPS = 1e-6


def rms_rel_r(D):
    """relative error of the kernel's r: a product passes 1 + 4 additions in its pass, one per later pass and the 10
    of the block sum; / D (2 U), + eps (U); the -1/2 power halves it; rsqrtf's own error on top."""
    passes = -(-D // 1024)
    return inv_sqrt_rel(gam(passes + 14) + 3 * U) * SECOND + RSQRT_REL


def rmsnorm_ref(x, g, eps, round_fp16, mut=()):
    """x [M][D], g [D] -> NS(y float64, and what accept_rms needs)"""
    x64, g64 = x.double(), g.double()
    D = x.shape[1]
    ms = (x64 * x64).sum(-1, keepdim=True) / ((D - 1) if "nm1" in mut else D)
    r = 1.0 / torch.sqrt(ms + (0.0 if "noeps" in mut else float(np.float32(eps))))
    h = x64 * r
    if "gshift" in mut:
        g64 = torch.roll(g64, 1)
    dh = h.abs() * (rms_rel_r(D) + U) * SECOND          # the kernel's float32 x * r lies within dh of h
    if not round_fp16 or "nofp16" in mut:
        return NS(y=g64 * h, E=(g64 * h).abs() * (rms_rel_r(D) + 2 * U) * SECOND, fp16=False)
    if "fp16late" in mut:
        return NS(y=f16_of_f64(g64 * h), E=None, fp16=False)
    h16, lo, hi = f16_of_f64(h), f16_of_f64(h - dh), f16_of_f64(h + dh)
    amb = lo != hi
    nb = torch.where(lo != h16, lo, hi)                  # the neighbouring fp16 value the kernel may land on
    g32 = g.float()
    return NS(y=g64 * h16, fp16=True, amb=amb, exact=g32 * h16.float(), alt=g32 * nb.float())


def accept_rms(got, ref):
    """-> worst err / E (plain), or 0.0 / inf (fp16: float32-exact g * fp16(x r), the neighbour where ambiguous)"""
    if not ref.fp16:
        if ref.E is None:
            return 0.0 if torch.equal(got.double(), ref.y) else math.inf
        return ratio(got, ref.y, ref.E)
    ok = (got == ref.exact) | (ref.amb & (got == ref.alt))
    return 0.0 if bool(ok.all()) else math.inf


def _rms_case(D, M, rf, inplace=False):
    name = f"rms/D{D}/M{M}/{'fp16' if rf else 'f32'}{'/inplace' if inplace else ''}"

    def build():
        g = gen(name)
        x = randn(g, M, D)
        if M == 3:
            x[1] *= 1e-4        # eps matters: mean square 1e-8 against eps 1e-6
            x[2] = 0.0
        return x, 1.0 + 0.1 * randn(g, D)
    ldx = D + 4
    return NS(name=name, D=D, M=M, rf=rf, inplace=inplace, ldx=ldx, ldo=ldx if inplace else D + 8, eps=RMS_EPS,
              build=build)


RMS_CASES = [_rms_case(D, M, rf) for D in (4, 252, 1024, 1028, 3584) for M in (1, 3) for rf in (False, True)] + \
            [_rms_case(D, 3, rf, inplace=True) for D in (252, 3584) for rf in (False, True)]


# ------------------------------------------------------------------------------------------------ layernorm
# k_layernorm: mean = block_sum(x) / D, var = block_sum((x - mean)^2) / D, r = 1 / sqrtf(var + eps),
# out = act((x - mean) * r * w + b).
GELU_LIP = 1.13      # sup |gelu'| = 1.1290


def _two_pass_bounds(x64, n_t, n, eps):
    """Errors of the two-pass statistics over the last axis: (mean, d = x - mean, var, dd >= |d_k - d|, rho_q: the
    relative error of the kernel's var + eps)."""
    mean = x64.mean(-1, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(-1, keepdim=True)
    dmean = gam(n_t + 10) * x64.abs().sum(-1, keepdim=True) / n + 2 * U * mean.abs()
    dd = (dmean + U * (d.abs() + dmean)) * SECOND
    dvar = ((2 * d.abs() * dd + dd * dd).sum(-1, keepdim=True)
            + gam(n_t + 11) * ((d.abs() + dd) ** 2).sum(-1, keepdim=True)) / n + 2 * U * var
    rho_q = (dvar + U * (var + eps)) / (var + eps)
    return mean, d, var, dd, rho_q * SECOND


def act64(v, act, tanh=False):
    if act == "relu":
        return torch.relu(v)
    if act == "gelu":
        if tanh:
            return 0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))
        return 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))
    return v


def act_bound(v, dv, act):
    """|act_k(v_k) - act(v)| for |v_k - v| <= dv.  ReLU is exact and 1-Lipschitz.  GELU 0.5 v (1 + erf(z)), z = v c:
    the argument's two roundings move erf by at most |z erf'(z)| 2 U <= 0.97 U; erff adds ERF_REL |erf|; 1 + erf one
    rounding; the two products 2 U."""
    if act != "gelu":
        return dv
    z = v / math.sqrt(2.0)
    t = 1 + torch.erf(z)
    dt = ERF_REL * torch.erf(z).abs() + 0.97 * U + U * t
    return GELU_LIP * dv + 0.5 * v.abs() * dt + 2 * U * act64(v, "gelu").abs()


def layernorm_ref(x, w, b, eps, act, mut=()):
    """-> (y, E) float64"""
    D = x.shape[1]
    x64, w64, b64 = x.double(), w.double(), b.double()
    eps = float(np.float32(eps))
    mean, d, var, dd, rho_q = _two_pass_bounds(x64, -(-D // 256), D, eps)
    r = 1.0 / torch.sqrt(var + eps)
    rho_r = inv_sqrt_rel(rho_q) + 4 * U          # sqrtf U, the division 2 U, and the halved + eps rounding's share
    v = d * r * w64 + b64
    dv = (w64.abs() * r * (dd + d.abs() * (rho_r + 3 * U)) + U * v.abs()) * SECOND
    E = act_bound(v, dv, act)
    if "unbiased" in mut:
        v = d / torch.sqrt(var * D / (D - 1) + eps) * w64 + b64
    if "onepass" in mut:
        x32 = x.float()
        v32 = (x32 * x32).mean(-1, keepdim=True) - x32.mean(-1, keepdim=True) ** 2
        v = d / torch.sqrt(v32.double() + eps) * w64 + b64
    if "actfirst" in mut:
        return act64(d * r, act) * w64 + b64, E
    return act64(v, act, tanh="tanh" in mut), E


def _ln_case(D, act, eps, inplace=False):
    name = f"ln/D{D}/{act}/eps{eps:g}{'/inplace' if inplace else ''}"

    def build():
        g = gen(name)
        x = randn(g, 4, D)
        x[1] = 0.75                                   # every partial sum exact: the variance is exactly 0
        x[2] = 100.0 + 1e-2 * randn(g, D)             # mean >> spread
        x[3] *= 3.0
        return x, 1.0 + 0.1 * randn(g, D), 0.5 * randn(g, D)
    ldx = D + 3
    return NS(name=name, D=D, M=4, act=act, eps=eps, inplace=inplace, ldx=ldx, ldo=ldx if inplace else D + 5,
              build=build)


LN_CASES = [_ln_case(D, act, eps) for i, D in enumerate((1, 255, 256, 257, 1024))
            for j, act in enumerate(("none", "relu", "gelu")) for eps in ((1e-5, 1e-3)[(i + j) % 2],)] + \
           [_ln_case(257, "gelu", 1e-3, inplace=True), _ln_case(1024, "relu", 1e-5, inplace=True),
            _ln_case(255, "none", 1e-5, inplace=True), _ln_case(1024, "gelu", 1e-3)]


# ------------------------------------------------------------------------------------------------ gather_rows
def gather_ref(table, idx, M, D, round_fp16):
    rows = table[:M] if idx is None else table[idx.long()]
    v = rows[:, :D].float()
    return v.half().float() if round_fp16 else v


def _gather_case(name, D, bf16=False, ld_extra=0, idx="perm", out_rows=False, rf=False, col0=0, M=5):
    def build():
        g = gen("gather/" + name)
        R = 9
        tab = randn(g, R, D + ld_extra) * 3.0
        tab = tab.bfloat16() if bf16 else tab
        ix = {"none": None, "perm": torch.tensor([8, 8, 3, 1, 0][:M] if M else [], dtype=torch.int32)}[idx]
        orow = torch.tensor([6, 0, 4, 3, 1][:M], dtype=torch.int32) if out_rows else None
        return tab, ix, orow          # the table's first D columns are the rows (ld_tab = D + ld_extra)
    return NS(name=name, D=D, M=M, bf16=bf16, rf=rf, col0=col0, out_R=8 if out_rows else max(M, 1), build=build)


GATHER_CASES = [
    _gather_case("f32/D1", 1), _gather_case("f32/D255/ld", 255, ld_extra=3), _gather_case("f32/D256/id", 256, idx="none"),
    _gather_case("f32/D257/rows", 257, out_rows=True), _gather_case("bf16/D255/fp16", 255, bf16=True, rf=True),
    _gather_case("bf16/D256/ld/rows", 256, bf16=True, ld_extra=8, out_rows=True),
    _gather_case("bf16/D257/id", 257, bf16=True, idx="none"), _gather_case("f32/D257/fp16/col", 257, rf=True, col0=5),
    _gather_case("bf16/D1/col", 1, bf16=True, col0=2), _gather_case("f32/D256/M0", 256, M=0),
]


# ------------------------------------------------------------------------------------------------ adapter streaming state
# k_im2col_conv1d: seq_b = [cache_b (KC rows); x_b (T rows)], out row (b, t) col c K + j = seq_b[S t + j][c], pad
# columns zero.  k_conv_cache_update: cache_b <- the last KC rows of x_b.  (models/adapter.py:124-143 of the
# reference: the chunk's conv runs over cat(cache, x) and keeps x[..., 1 - K:].)
def im2col_ref(cache, x, K, S, ldo, mut=()):
    """cache [B][KC][D] (None: zeros), x [B][T][D] -> [B * To][ldo]"""
    B, T, D = x.shape
    KC = K - 1
    c = torch.zeros(B, KC, D, dtype=x.dtype) if cache is None else cache
    if "cacheshift" in mut:
        c = torch.roll(c, 1, dims=1)
    seq = torch.cat([c, x], 1)
    S_ = 1 if "nostride" in mut else S
    To = (KC + T - K) // S + 1
    out = torch.zeros(B, To, ldo, dtype=x.dtype)
    for t in range(To):
        win = seq[:, S_ * t:S_ * t + K]                      # [B][K][D]
        out[:, t, :D * K] = (win.reshape(B, K * D) if "colorder" in mut
                             else win.transpose(1, 2).reshape(B, D * K))
    return out.reshape(B * To, ldo)


def cache_ref(x, KC, mut=()):
    return x[:, :KC].clone() if "first" in mut else x[:, x.shape[1] - KC:].clone()


def stream_conv64(xs, w, K, S):
    """One causal strided conv over the concatenated stream (KC zeros in front): xs [B][Ttot][D], w [Co][D][K]"""
    return F.conv1d(F.pad(xs.double().transpose(1, 2), (K - 1, 0)), w.double(), stride=S).transpose(1, 2)


def _stream_case(K, S, T, D, pad, slots, null_first):
    name = f"stream/K{K}/S{S}/T{T}/D{D}/{'pad' if pad else 'tight'}/{'slots' if slots else 'ident'}" \
           f"{'/null' if null_first else ''}"

    def build():
        g = gen(name)
        return [randn(g, 2, T, D) for _ in range(3)], randn(g, 4, D, K).double()
    return NS(name=name, K=K, S=S, T=T, D=D, B=2, KC=K - 1, ldo=D * K + (5 if pad else 0),
              slots=[3, 1] if slots else None, pool=5 if slots else 2, null_first=null_first, build=build)


STREAM_CASES = [_stream_case(K, S, T, D, pad=(i + j) % 2 == 0, slots=(i // 2 + j) % 2 == 0, null_first=i % 3 == 0)
                for i, (K, S, T) in enumerate((K, S, T) for K in (3, 5) for S in (1, 2)
                                              for T in (K - 1, K, 7, 8))
                for j, D in enumerate((3, 64))]


def stream_model(case, mut_im=(), mut_cache=()):
    """-> per chunk (cols, cache after) from the model, and the stream check: cols @ w against one conv over the
    stream (asserted by the caller when T % S == 0; an odd chunk under stride 2 restarts the stride's phase, in
    the reference as here)."""
    xs, w = case.build()
    cache = None
    out = []
    for x in xs:
        cols = im2col_ref(cache, x, case.K, case.S, case.ldo, mut_im)
        cache = cache_ref(x, case.KC, mut_cache)
        out.append((cols, cache))
    return xs, w, out


def stream_property(case, xs, w, cols_list):
    """max |chunked - whole| / bound, bound = 2^-40 sum |w| |x| (float64 sums of at most 320 products in two orders)"""
    B, Co = case.B, w.shape[0]
    wm = w.reshape(Co, case.D * case.K)
    ys = [(c[:, :case.D * case.K].double() @ wm.t()).reshape(B, -1, Co) for c in cols_list]
    whole = stream_conv64(torch.cat(xs, 1), w, case.K, case.S)
    a = stream_conv64(torch.cat(xs, 1).abs(), w.abs(), case.K, case.S)
    got = torch.cat(ys, 1)
    if got.shape != whole.shape:
        return math.inf
    return float(((got - whole).abs() / (2.0 ** -40 * a + 1e-300)).max())


# ------------------------------------------------------------------------------------------------ fill_hash
def hash_ref(key, n, center, scale):
    """oracle/weights.py hash_uniform for a raw 64-bit key: the bf16-rounded values as float32 [n]"""
    out = np.empty(n, dtype=np.float32)
    for i0 in range(0, n, 1 << 22):
        idx = np.arange(i0, min(n, i0 + (1 << 22)), dtype=np.uint64)
        with np.errstate(over="ignore"):
            v = ow._splitmix64_np(np.uint64(key) + idx)
        u = (v >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
        w = ((np.float32(2.0) * u - np.float32(1.0)) * np.float32(scale) + np.float32(center)).astype(np.float32)
        out[i0:i0 + len(w)] = ow.bf16_round(w)
    return torch.from_numpy(out)


HASH_N_BIG = 8192 * 256 + 3          # one past grid_for's cap of 8192 blocks of 256: the grid-stride loop runs
HASH_CASES = [NS(name="f32/big", n=HASH_N_BIG, bf16=False, key=0x1234567890ABCDEF, center=0.0, scale=0.5),
              NS(name="bf16/big/wrap", n=HASH_N_BIG, bf16=True, key=(1 << 64) - (1 << 19), center=1.0, scale=0.1),
              NS(name="f32/scale0", n=257, bf16=False, key=99, center=0.3, scale=0.0),
              NS(name="bf16/small", n=5, bf16=True, key=(1 << 64) - 2, center=0.0, scale=1.0),
              NS(name="f32/n0", n=0, bf16=False, key=7, center=0.0, scale=1.0)]


# ================================================================================================ B. fo_fbank
# k_fbank per (user, frame): mean removal, pre-emphasis 0.97 (x[-1] = x[0]), window, zero pad, radix-2 FFT with the
# launch's twiddle tables, |X|^2, mel rows, log(max(e, FLT_EPSILON)).
PRE32 = float(np.float32(0.97))


def fft_tables64(y, tw_cos, tw_sin):
    """The kernel's decimation-in-time FFT in float64 with the given (float32) tables: y [..., nfft] real ->
    (re, im) [..., nfft]"""
    n = y.shape[-1]
    log2n = n.bit_length() - 1
    rev = np.array([int(format(i, f"0{log2n}b")[::-1], 2) for i in range(n)])
    re, im = np.zeros_like(y), np.zeros_like(y)
    re[..., rev] = y
    c64, s64 = tw_cos.astype(y.dtype), tw_sin.astype(y.dtype)   # (float32 y: the CPU test's stand-in kernel)
    k = np.arange(n // 2)
    m = 1
    while m < n:
        grp, pos = k // m, k % m
        i0 = grp * 2 * m + pos
        i1 = i0 + m
        t = pos * (n // (2 * m))
        c, s = c64[t], s64[t]
        xr = re[..., i1] * c + im[..., i1] * s
        xi = im[..., i1] * c - re[..., i1] * s
        ar, ai = re[..., i0].copy(), im[..., i0].copy()
        re[..., i0], im[..., i0], re[..., i1], im[..., i1] = ar + xr, ai + xi, ar - xr, ai - xi
        m *= 2
    return re, im


def fbank_ref(samples, n_samples, wl, ws, nfft, window, tw_cos, tw_sin, mel, mut=()):
    """samples [B][>= n_samples] float32, tables float32 numpy -> (log-mel [B][frames][nmel], bound) float64.
    Bound per mel energy: per bin |dX_k| <= sum_n dy_n + 4 log2(nfft) U ||y||_1 -- a term of the FFT passes log2(nfft)
    butterflies, each a complex product by a unit twiddle (2 sqrt 2 U of its magnitude) and an addition (U); with
    ||y||_1 <= sqrt(wl) ||y||_2 this is c log2(nfft) U ||y||_2, c = 4 ||y||_1 / ||y||_2 <= 4 sqrt(wl) -- where dy_n
    is the error of the windowed sample: both taps subtract the same computed mean, so its error (wl / 256 terms a
    thread + 10, then the division) passes with the factor 1 - 0.97 only; the two subtractions round at U |x - mean|
    each, the product by 0.97 and the difference once more, then the window product.  Then |d|X|^2| <= 2 |X| dX + dX^2 +
    3 U |X|^2, the mel row's sequential sum over its nz non-zero weights gam(nz + 1) e, and in the log domain
    r / (1 - r) with r = dE / max(e, eps), + LOG_REL |log|."""
    x = samples[:, :n_samples].astype(np.float64)
    B = x.shape[0]
    frames = 1 + (n_samples - wl) // ws
    fr = np.stack([x[:, f * ws:f * ws + wl] for f in range(frames)], 1)          # [B][frames][wl]
    mean = fr.mean(-1, keepdims=True)
    dmean = gam(-(-wl // 256) + 10) * np.abs(fr).sum(-1, keepdims=True) / wl + 2 * U * np.abs(mean)
    if "nomean" in mut:
        mean = np.zeros_like(mean)
    xi = fr - mean
    prev = np.concatenate([fr[..., :1], fr[..., :-1]], -1) - mean
    if "pre0" in mut:
        prev[..., 0] = 0.0
    win = window.astype(np.float64)
    if "hann" in mut:
        n = np.arange(wl, dtype=np.float64)
        win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (wl - 1))
    a, b = np.abs(xi), PRE32 * np.abs(prev)
    yw = (xi - PRE32 * prev) * win
    dy = (win * (0.031 * dmean + U * (a + 2 * b + np.abs(xi - PRE32 * prev))) + U * np.abs(yw)) * SECOND
    y = np.zeros((B, frames, nfft))
    y[..., :wl] = yw
    re, im = fft_tables64(y, tw_cos, tw_sin)
    nb = nfft // 2 + 1
    X2 = (re * re + im * im)[..., :nb]
    log2n = nfft.bit_length() - 1
    dX = dy.sum(-1, keepdims=True) + 4 * log2n * U * np.abs(yw).sum(-1, keepdims=True) * SECOND
    dP = 2 * np.sqrt(X2) * dX + dX * dX + 3 * U * X2
    mel64 = mel.astype(np.float64)
    if "melshift" in mut:
        mel64 = mel64.copy()
        mel64[40] = np.roll(mel64[40], 1)
    e = X2 @ mel64.T
    nz = (mel != 0).sum(-1)
    dE = dP @ mel.astype(np.float64).T + gam(nz + 1) * e
    if "logadd" in mut:
        return np.log(e + FLT_EPS), None
    r = dE / np.maximum(e, FLT_EPS)
    out = np.log(np.maximum(e, FLT_EPS))
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.where(r < 1, r / (1 - r), np.inf) + LOG_REL * np.abs(out)
    return out, bound


def fbank_tables(framing):
    from fo.tables import kaldi_tables
    wl, nfft = {"A": (400, 512), "B": (256, 256)}[framing]
    ws = {"A": 160, "B": 128}[framing]
    return (wl, ws, nfft) + tuple(t.numpy() for t in kaldi_tables(wl, nfft))


FB_CEIL = 1e-3     # the inputs are chosen so that every compared element's bound stays below this


def _fb_signal(g, B, n):
    """Noise plus tones at int16 scale, shaped so that no mel band is starved against ||y||: the noise is an AR(1)
    process with the pre-emphasis' own pole (white after it), and the tones are a comb at the multiples of 62.5 Hz up
    to 1.5 kHz, each 100 / |1 - 0.97 exp(-i w)| high (100 after the pre-emphasis) -- the low mel triangles hold one
    or two FFT bins, and a bin of noise alone is Rayleigh-distributed and now and then nearly empty."""
    e = randn(g, B, n + 200).numpy().astype(np.float64) * 300.0
    x = np.zeros_like(e)
    for i in range(1, e.shape[1]):
        x[:, i] = 0.97 * x[:, i - 1] + e[:, i]
    x = x[:, 200:]
    t = np.arange(n)
    ph = torch.rand(B, 24, generator=g).numpy() * 2 * np.pi
    for k in range(1, 25):
        w = 2 * np.pi * 62.5 * k / 16000.0
        x = x + (100.0 / abs(1 - 0.97 * np.exp(-1j * w))) * np.sin(w * t[None] + ph[:, k - 1:k])
    assert np.abs(x).max() < 32768
    return x.astype(np.float32)


def _fb_case(name, framing, frames, B=1, ld_extra=0, row0=0, zero_rows=None, kind="signal", flat=False):
    def build():
        wl, ws, nfft, window, twc, tws, mel = fbank_tables(framing)
        if flat:     # a window that does not vanish at its ends (Povey's first tap is 0 and hides x[-1])
            window = (0.5 + 0.5 * window).astype(np.float32)
        n = wl + (frames - 1) * ws
        for attempt in range(64):            # the first seed whose bound stays under the ceiling
            g = gen(f"fbank/{name}/{attempt}")
            if kind == "zero":
                s = np.zeros((B, n), np.float32)
            elif kind == "faint":          # mel energies around FLT_EPSILON: the clamp is not an addition
                s = _fb_signal(g, B, n) * np.float32(3e-8)
            elif kind == "dc":
                s = np.full((B, n), 1000.0, np.float32)
            else:
                s = _fb_signal(g, B, n)
            want, bound = fbank_ref(s, n, wl, ws, nfft, window, twc, tws, mel)
            if kind in ("zero", "dc") or bound.max() < FB_CEIL:
                break
        buf = np.full((B, n + ld_extra), 3.0e4, np.float32)     # the tail past n_samples must never reach a frame
        buf[:, :n] = s
        return NS(samples=buf, n=n, want=want, bound=bound, tables=(wl, ws, nfft, window, twc, tws, mel))
    return NS(name=name, framing=framing, frames=frames, B=B, row0=row0, zero_rows=zero_rows, kind=kind, build=build)


FBANK_CASES = [
    _fb_case("A/one", "A", 1), _fb_case("B/one", "B", 1), _fb_case("A/four", "A", 4), _fb_case("B/five", "B", 5),
    _fb_case("A/B3/ld", "A", 3, B=3, ld_extra=171), _fb_case("B/B3/ld/row0", "B", 3, B=3, ld_extra=64, row0=2),
    _fb_case("A/zero_rows", "A", 3, B=3, zero_rows=[0, 1, 3], ld_extra=5, row0=1),
    _fb_case("A/flatwin", "A", 2, flat=True), _fb_case("A/faint", "A", 2, kind="faint"), _fb_case("A/zeros", "A", 2, kind="zero"), _fb_case("B/dc", "B", 2, kind="dc"), _fb_case("A/dc", "A", 2, kind="dc"),
]


# ================================================================================================ C. silence cut
# k_silence_cut (find_min_sum_index, models/decoder/llm2tts.py:91-103 of the reference): window sums of |x| in
# double, CAST TO FLOAT, first minimum from start = L // 2 - N // 2; s0 = max(0, mi + start), e0 = min(L, mi + N +
# s0); first arg-min of |x| in [s0, e0).  The float cast decides ties: two windows whose double sums differ by less
# than a float ulp tie, and the first wins.
def silence_ref(x, N, mut=()):
    """x float32 [L] numpy -> (min_sum float32, cut int)"""
    L = len(x)
    a = np.abs(x.astype(np.float64))
    P = np.concatenate([[0.0], np.cumsum(a)])
    start = ((L + 1) // 2 if "mid" in mut else L // 2) - N // 2
    sums = P[start + N:L + 1] - P[start:L - N + 1]
    if not len(sums):          # (only a mutant's start can leave no window)
        return np.float32("nan"), -1
    s32 = sums if "double" in mut else sums.astype(np.float32)
    mi = int(len(s32) - 1 - np.argmin(s32[::-1])) if "last" in mut else int(np.argmin(s32))
    s0 = max(0, mi + start)
    e0 = min(L, mi + N + (start if "e0" in mut else s0))
    cut = s0 + int(np.argmin(np.abs(x[s0:e0])))
    return np.float32(sums[mi]), cut


def _dy_noise(g, L, lo=8):
    """multiples of 2^-6 with lo / 64 <= |x| < 4: every window sum is exact in float32 (< 2^18 with 6 fraction bits)"""
    m = torch.randint(lo, 256, (L,), generator=g).numpy().astype(np.float32) / 64.0
    sg = torch.randint(0, 2, (L,), generator=g).numpy().astype(np.float32) * 2 - 1
    return m * sg


def _dy(name, L, N, edit=None):
    def build():
        x = _dy_noise(gen("sil/" + name), L)
        if edit:
            edit(x, L, N, L // 2 - N // 2)
        return x
    return NS(name=name, L=L, N=N, build=build)


def _quiet(x, at, n, v=1.0 / 64):
    x[at:at + n] = v * np.where(np.arange(n) % 2, -1.0, 1.0).astype(np.float32)


def _e_two(x, L, N, st):          # two equally quiet stretches: the first wins
    _quiet(x, st + 100, N)
    _quiet(x, st + 300, N)


def _e_zeros(x, L, N, st):        # zeros for longer than N: many windows sum to exactly 0
    x[st + 200:st + 200 + N + 100] = 0.0


def _e_first(x, L, N, st):
    _quiet(x, st, N)


def _e_last(x, L, N, st):
    _quiet(x, L - N, N)


def _e_argmin(x, L, N, st):
    """the quietest window at st + 10 holds |x| = 2/64 but for three samples of 1/64, 1030 and 2100 apart (threads
    5, 11 and 57 of the arg-min's 1024): the first wins"""
    _quiet(x, st + 10, N, 2.0 / 64)
    for o in (2105, 1035, 5):
        x[st + 10 + o] = -1.0 / 64


def _e_beyond(x, L, N, st):
    """the quietest window at st + 100 is followed, 20 samples after its end and inside [s0, e0), by a zero: the cut"""
    _quiet(x, st + 100, N, 2.0 / 64)
    x[st + 100 + N + 20] = 0.0


def _e_prefix(x, L, N, st):
    _quiet(x, 20000, N)
    x[20000 + 77] = 0.0


def _cast_tie():
    """L 9, N 4 (start 2): windows 0 and 1 sum to 1201 and 1201 - 2^-16, equal as floats (ulp 2^-13): the kernel
    takes window 0 and cuts at 2; an arg-min over the double sums takes window 1 and cuts at 6."""
    x = np.array([500, 500, 1, 400, 400, 400, 1 - 2.0 ** -16, 500, 500], np.float32)
    return NS(name="cast-tie/L9/N4", L=9, N=4, build=lambda: x.copy())


SC_MAX_STAGE = 36798     # csrc/fo_codec.hip: the longest row k_silence_cut stages in LDS


def _prefix_pair():
    """Rows sharing one prefix either side of the staging boundary, and at 36862 / 36863: 36862 is the length whose
    staged launch asked for 8 bytes more LDS than a workgroup has and aborted the queue (the boundary was (160 KB -
    static LDS) / 4 without the dynamic array's alignment padding); it is read from global memory now."""
    a = _dy("L36863/N2401/unstaged", 36863, 2401, _e_prefix)

    def cut(L, kind):
        return NS(name=f"L{L}/N2401/{kind}", L=L, N=2401, build=lambda: a.build()[:L].copy())
    return [cut(SC_MAX_STAGE, "staged"), cut(SC_MAX_STAGE + 1, "unstaged"), cut(36862, "unstaged"), a]


SIL_EXACT = [
    _dy("zeros/L4097/N2401", 4097, 2401, lambda x, L, N, st: x.fill(0.0)),
    _dy("L9/N4", 9, 4), _dy("L10/N5", 10, 5), _dy("L5/N5", 5, 5), _dy("L2401/N2401", 2401, 2401),
    _dy("two/L1023/N64", 1023, 64, _e_two), _dy("zerorun/L1024/N64", 1024, 64, _e_zeros),
    _dy("first/L1025/N64", 1025, 64, _e_first), _dy("last/L4097/N2401", 4097, 2401, _e_last),
    _dy("argmin/L6000/N2401", 6000, 2401, _e_argmin), _dy("last/L1023/N64", 1023, 64, _e_last),
    _dy("beyond/L1024/N64", 1024, 64, _e_beyond), _cast_tie(),
] + _prefix_pair()
SIL_ROWS = NS(name="rows/L4097/N2401", L=4097, N=2401, ld=4097 + 37,
              build=lambda: np.stack([_dy(f"row{r}", 4097, 2401, e).build() for r, e in
                                      enumerate((_e_two, _e_last, None))]))


def silence_gap_ulps(x, N):
    """float ulps between the best window's float32 sum and the least one outside its +-1 neighbourhood"""
    L = len(x)
    P = np.concatenate([[0.0], np.cumsum(np.abs(x.astype(np.float64)))])
    start = L // 2 - N // 2
    s32 = (P[start + N:L + 1] - P[start:L - N + 1]).astype(np.float32)
    mi = int(np.argmin(s32))
    rest = np.delete(s32, [i for i in (mi - 1, mi, mi + 1) if 0 <= i < len(s32)])
    return math.inf if not len(rest) else float((rest.min() - s32[mi]) / np.spacing(s32[mi]))


def _sil_random(name, L, N):
    def build():
        for attempt in range(64):        # the first seed whose best window is clear of the runner-up
            g = gen(f"silrand/{name}/{attempt}")
            x = (randn(g, L) * 0.05).numpy()
            q = L // 2 + int(torch.randint(0, max(1, L // 2 - N - N // 2), (1,), generator=g))
            x[q:q + N + 300] *= 1e-3
            if silence_gap_ulps(x, N) >= 4:
                return x
        raise AssertionError(name)
    return NS(name=name, L=L, N=N, build=build)


SIL_RANDOM = [_sil_random("L4097/N2401", 4097, 2401), _sil_random("L40000/N2401", 40000, 2401),
              _sil_random("L1500/N64", 1500, 64)]


# ================================================================================================ D. fo_codec_enc.hip
# ------------------------------------------------------------------------------------------------ conv1d_ex
def leaky(x, slope):
    return torch.where(x < 0, x * slope, x)


def conv_ex_ref(x, w, bias, stride, dil, pad, slope, prefill, mut=()):
    """x [B][Cin][Tin], w [Cout][Cin][K] -> (y, E) [B][Cout][Tout]:
    E = (Cin K + 2) U sum |w| |act(x)| + U |out|  (Cin K fma accumulations, the slope product, the bias add; the
    stored value's own rounding, the residual add included)."""
    x64, w64 = x.double(), w.double()
    if slope is not None:
        x64 = leaky(x64, float(np.float32(slope)))
    K = w.shape[2]
    wq = torch.flip(w64, dims=[2]) if "flip" in mut else w64
    if "dilstride" in mut:
        y = F.conv1d(x64, wq, None, stride=dil, dilation=dil, padding=pad)
        Tout = (x.shape[2] + 2 * pad - dil * (K - 1) - 1) // stride + 1
        y = F.pad(y, (0, max(0, Tout - y.shape[2])))[..., :Tout]
    else:
        y = F.conv1d(x64, wq, None, stride=stride, dilation=dil, padding=pad)
    A = F.conv1d(x64.abs(), w64.abs(), None, stride=stride, dilation=dil, padding=pad)
    if bias is not None:
        y = y + bias.double()[None, :, None]
    if prefill is not None:
        y = y + prefill.double()
    return y, (x.shape[1] * K + 2) * U * A + U * y.abs()


def _conv_case(name, Cin, Cout, K, stride, dil, pad, Tout, bias=True, slope=None, residual=False, B=2):
    reach = dil * (K - 1)
    p = {"same": reach // 2, "big": reach + 3}.get(pad, pad)
    Tin = (Tout - 1) * stride + reach + 1 - 2 * p
    assert Tin > 0, name

    def build():
        g = gen("convex/" + name)
        return NS(x=randn(g, B, Cin, Tin), w=randn(g, Cout, Cin, K) / math.sqrt(Cin * K),
                  bias=0.05 * randn(g, Cout) if bias else None,
                  prefill=randn(g, B, Cout, Tout) if residual else None)
    return NS(name=name, B=B, Cin=Cin, Cout=Cout, K=K, stride=stride, dil=dil, pad=p, Tin=Tin, Tout=Tout, slope=slope,
              residual=residual, build=build)


# (a residual case keeps its bias small against the taps it meets, or has none: the bias add's own rounding is the
#  second of the "+ 2")
CONVEX_CASES = [
    _conv_case("c1/k1", 1, 1, 1, 1, 1, 0, 127),
    _conv_case("c1/k1/res", 1, 3, 1, 1, 1, 0, 5, bias=False, residual=True),
    _conv_case("c5/k3/same", 5, 3, 3, 1, 1, "same", 128, slope=0.1),
    _conv_case("c5/k7/s2", 5, 3, 7, 2, 1, "same", 129, slope=0.01),
    _conv_case("c32/k7/d3/same", 32, 3, 7, 1, 3, "same", 129, slope=0.1, residual=True),
    _conv_case("c32/k3/d5/same/nobias", 32, 1, 3, 1, 5, "same", 127, bias=False, slope=0.1),
    _conv_case("c32/k11/s5/big", 32, 3, 11, 5, 1, "big", 128, slope=0.1),
    _conv_case("c5/k11/d3/big", 5, 1, 11, 1, 3, "big", 70),
    _conv_case("c1/k3/s5/T1", 1, 3, 3, 5, 1, 0, 1),
    _conv_case("c5/k7/s2/d5/pad0", 5, 3, 7, 2, 5, 0, 1, slope=0.01),
    _conv_case("c32/k1/s2/nobias/res", 32, 3, 1, 2, 1, 0, 129, bias=False, residual=True),
    _conv_case("c5/k3/d3/same/T1", 5, 1, 3, 1, 3, "same", 1, slope=0.1),
]


# ------------------------------------------------------------------------------------------------ group_norm
def group_norm_ref(x, G, w, b, eps, scale, mut=()):
    """x [B][C][T] -> (y, E): k_group_norm's two-pass statistics over a group's C / G * T elements (256 threads),
    rstd = rsqrtf(var + eps), out = ((x - mean) rstd w + b) scale."""
    B, C, T = x.shape
    cg = C // G
    n = cg * T
    x64 = x.double().reshape(B, G, n)
    eps = float(np.float32(eps))
    mean, d, var, dd, rho_q = _two_pass_bounds(x64, -(-n // 256), n, eps)
    if "perchannel" in mut:
        xc = x.double()
        mc = xc.mean(-1, keepdim=True)
        vc = ((xc - mc) ** 2).mean(-1, keepdim=True)
        return ((xc - mc) / torch.sqrt(vc + eps) * w.double()[None, :, None] + b.double()[None, :, None]) * scale, None
    r = 1.0 / torch.sqrt(var + eps)
    rho_r = inv_sqrt_rel(rho_q) + RSQRT_REL
    w64 = w.double().reshape(1, G, cg, 1).expand(B, G, cg, T).reshape(B, G, n)
    b64 = b.double().reshape(1, G, cg, 1).expand(B, G, cg, T).reshape(B, G, n)
    v = d * r * w64 + b64
    dv = (w64.abs() * r * (dd + d.abs() * (rho_r + 3 * U)) + U * v.abs()) * SECOND
    sc = float(np.float32(scale))
    return (v * sc).reshape(B, C, T), ((dv * abs(sc) + U * (v * sc).abs()) * SECOND).reshape(B, C, T)


def _gn_case(G, T, scale, inplace=False):
    name = f"gn/G{G}/T{T}/s{'1' if scale == 1.0 else '3rd'}{'/inplace' if inplace else ''}"

    def build():
        g = gen(name)
        C = 16 * G
        x = randn(g, 3, C, T)
        x[1, :16] = 0.75                                       # a constant group: the output is exactly bias * scale
        x[2, C - 16:] = 100.0 + 1e-2 * randn(g, 16, T)         # mean >> spread
        return x, 1.0 + 0.1 * randn(g, C), 0.5 * randn(g, C)
    return NS(name=name, G=G, C=16 * G, T=T, B=3, eps=1e-6, scale=scale, inplace=inplace, build=build)


GN_CASES = [_gn_case(G, T, (1.0, THIRD)[(i + j) % 2]) for i, G in enumerate((1, 2, 4)) for j, T in enumerate((1, 7, 300))] \
           + [_gn_case(2, 300, THIRD, inplace=True), _gn_case(4, 7, 1.0, inplace=True), _gn_case(1, 300, THIRD)]


# ------------------------------------------------------------------------------------------------ gte_head
def gte_ref(x, lw, lb, rm, rv, bw, bb, eps, mut=()):
    """x [B][C][T] -> (y, E) [B][C]: v = mean_t leaky(x) (T additions, the slope product, the division: gam(T + 3));
    y = lb + sum_j lw v (C fma in a chain); leaky; (y - rm) rsqrtf(rv + eps) bw + bb."""
    B, C, T = x.shape
    lx = leaky(x.double(), SLOPE32)
    v = lx.mean(-1)
    dv = gam(T + 3) * lx.abs().mean(-1)
    lw64, lb64 = lw.double(), lb.double()
    y = v @ lw64.t() + lb64
    dy = dv @ lw64.abs().t() + gam(C + 1) * (v.abs() @ lw64.abs().t() + lb64.abs())
    r = 1.0 / torch.sqrt(rv.double() + float(np.float32(eps)))
    if "leakylast" in mut:
        return leaky((y - rm.double()) * r * bw.double() + bb.double(), SLOPE32), None
    yl = leaky(y, SLOPE32)
    dyl = dy + U * yl.abs()                       # leaky is 1-Lipschitz; its product rounds once
    z = yl - rm.double()
    out = z * r * bw.double() + bb.double()
    rho = U + RSQRT_REL                           # rv + eps, rsqrtf
    E = ((r * bw.double().abs()) * (dyl + z.abs() * (rho + 3 * U)) + U * out.abs()) * SECOND
    return out, E


def _gte_case(C, T):
    name = f"gte/C{C}/T{T}"

    def build():
        g = gen(name)
        rv = torch.rand(C, generator=g) * 0.6 + 0.7
        rv[::3] = torch.rand(len(rv[::3]), generator=g) * 1e-6       # near 0: bn_eps carries the scale
        return NS(x=randn(g, 2, C, T), lw=randn(g, C, C) / math.sqrt(C), lb=0.3 * randn(g, C), rm=0.1 * randn(g, C),
                  rv=rv, bw=1.0 + 0.1 * randn(g, C), bb=0.05 * randn(g, C))
    return NS(name=name, C=C, T=T, B=2, eps=1e-5, build=build)


GTE_CASES = [_gte_case(C, T) for C in (1, 96, 128, 1024) for T in (1, 5)]


# ------------------------------------------------------------------------------------------------ vq_nearest
def vq_err(x, E):
    """Bound on the float32 error of d_j = (xx + ee_j) - 2 xe_j, per (row, code): xx a block sum of products over
    D / 256 terms a thread, ee and xe chains of D fma, then two roundings.  x [R][D], E [n][D] float64."""
    D = x.shape[1]
    xx = (x * x).sum(-1, keepdim=True)
    ee = (E * E).sum(-1)[None]
    axe = x.abs() @ E.abs().t()
    d = xx + ee - 2 * x @ E.t()
    return (gam(-(-D // 256) + 11) * xx + gam(D) * ee + U * (xx + ee) + 2 * gam(D) * axe + U * d.abs()) * SECOND, d


def vq_ref(x, E, mut=()):
    """-> (ids [R], gap [R]: the next distinct code's distance minus the best, err [R]: the greatest bound of the row).
    Bit-identical codebook rows are one code to the model -- the kernel computes their distances identically, a
    float64 matrix product need not -- and the lowest index of the best code's copies is the answer."""
    Eu, first, inv = np.unique(E.numpy(), axis=0, return_index=True, return_inverse=True)
    last = np.zeros_like(first)
    np.maximum.at(last, inv.reshape(-1), np.arange(E.shape[0]))
    Eu = torch.from_numpy(Eu).double()
    err, d = vq_err(x.double(), Eu)
    if "noee" in mut:
        d = d - (Eu ** 2).sum(-1)[None]
    best = d.argmin(-1)
    ids = torch.from_numpy((last if "last" in mut else first)[best.numpy()])
    two = torch.topk(d, min(2, d.shape[1]), dim=-1, largest=False).values
    gap = two[:, -1] - two[:, 0] if d.shape[1] > 1 else torch.full((d.shape[0],), math.inf, dtype=torch.float64)
    return ids.int(), gap, err.max(-1).values


def vq_residual32(v, e):
    """the kernel's straight-through residual v - (v + (e - v)), each operation in float32"""
    return v - (v + (e - v))


def _vq_case(D, n_codes, T, residual):
    name = f"vq/D{D}/n{n_codes}/T{T}/{'res' if residual else 'ids'}"
    dups = [(7, 263), (300, 513), (0, n_codes - 1)] if n_codes >= 1024 else ([(0, n_codes - 1)] if n_codes > 1 else [])

    def build():
        g = gen(name)
        B, Ctot, ch0 = 2, D + 5, 3
        E = randn(g, n_codes, D) * (0.5 + 0.5 * (torch.arange(n_codes) % 3))[:, None]
        for lo, hi in dups:
            E[hi] = E[lo]                                   # bit-identical rows: the lower index must win
        R = B * T
        pool = [hi for _, hi in dups] + [lo for lo, _ in dups] + \
            [int(i) for i in torch.randint(0, n_codes, (R,), generator=g)]
        tgt = torch.tensor(pool[:R])
        rows = E[tgt] + 0.01 * randn(g, R, D)
        x = randn(g, B, Ctot, T)
        x[:, ch0:ch0 + D] = rows.reshape(B, T, D).transpose(1, 2)
        return NS(x=x, E=E, rows=rows, tgt=tgt, Ctot=Ctot, ch0=ch0, B=B)
    return NS(name=name, D=D, n_codes=n_codes, T=T, residual=residual, dups=dups, ids_ld=3, ids_col=1, build=build)


VQ_CASES = [_vq_case(D, n, T, res) for i, (D, n) in enumerate(((512, 1024), (64, 1024), (8, 1), (8, 255), (8, 257)))
            for T, res in (((1, False), (5, True)) if i % 2 == 0 else ((1, True), (5, False)))]
