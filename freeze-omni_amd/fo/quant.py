"""CPU reference of the weight-only FP8 quantiser (include/fo_hip.h fo_quant_w8): the definition of the
`mlp_weights="fp8"` model, used by tests and docs.  torch on the host only; the engine quantises on the device.

    W'[n, k] = q[n, k] * 2^e[n]

q is an OCP e4m3fn code (gfx950's format), e[n] one integer per output row: the smallest with
max|W[n, :]| * 2^-e[n] <= 448, taken from the float's exponent and mantissa (448 = 1.75 * 2^8), 0 for an all-zero row.
W * 2^-e is exact, so the rounding to e4m3fn (nearest-even) never saturates; q * 2^e has at most 4 significant bits and
is therefore exactly a bf16 value.

Below it, the same for the weight-only MXFP4 quantiser (fo_quant_w4, `mlp_weights="mxfp4"`): e2m1 codes with one
exponent per block of 32 columns; and for the weight-only MXFP6 quantiser (fo_quant_w6, `mlp_weights="mxfp6"`): e2m3
codes under the same block scales.
"""
import torch

# ---------------------------------------------------------------- the options and the formats each of them takes
# The one place the lists live: the engines, the weight sources, the facades and the command lines all check an option
# through check_format and build their `choices=` from FORMATS.
WEIGHT_FORMATS = ("fp8", "mxfp4", "mxfp6")      # the weight-only formats (ops.QUANT_FORMATS holds their layouts)
ATTN_WEIGHT_FORMATS = ("fp8", "mxfp4")          # ... those the fused q|k|v + RoPE GEMM is built for
FORMATS = {"mlp_weights": ("bf16",) + WEIGHT_FORMATS,
           "lm_head_weights": ("bf16",) + WEIGHT_FORMATS,
           "attn_weights": ("bf16",) + ATTN_WEIGHT_FORMATS,
           "llm_kv": ("fp32", "bf16", "e4m3"),
           "llm_rows_x": ("fp32", "bf16"),
           "FakeQuantSource format": WEIGHT_FORMATS,
           "FakeQuantSource lm_head": (None,) + WEIGHT_FORMATS,
           "FakeQuantSource attn": (None,) + ATTN_WEIGHT_FORMATS}


def check_format(option, value, allowed=None):
    """Raise ValueError("<option> must be 'a', 'b' or 'c', got <value>") unless `value` is one of `allowed` (default:
    FORMATS[option]); returns the value."""
    allowed = FORMATS[option] if allowed is None else allowed
    if value not in allowed:
        names = [repr(a) for a in allowed]
        raise ValueError(f"{option} must be {' or '.join(filter(None, (', '.join(names[:-1]), names[-1])))}, "
                         f"got {value!r}")
    return value


E4M3_MAX = 448.0


def row_exponents(w):
    """e[n] (int32) of a [N, K] weight."""
    amax = w.detach().float().abs().amax(dim=1)
    bits = amax.contiguous().view(torch.int32)
    e = (bits >> 23) - 127 - 8 + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)
    e = e.clamp(min=-126)            # 2^e and 2^-e stay normal floats
    return torch.where(amax > 0, e, torch.zeros_like(e))


def quantize_rows_e4m3(w):
    """w [N, K] (bf16 or fp32, CPU) -> (q uint8 [N, K] e4m3fn codes, e int32 [N], w_dq bf16 [N, K] = q * 2^e)."""
    w32 = w.detach().float()
    e = row_exponents(w32)
    scaled = torch.ldexp(w32, -e[:, None])
    q = scaled.to(torch.float8_e4m3fn)
    w_dq = torch.ldexp(q.float(), e[:, None]).to(torch.bfloat16)
    return q.view(torch.uint8), e, w_dq


def quantize_kv_rows(x):
    """The CPU model of the FP8 KV cache (llm_kv="e4m3"; fo_kv8_append): x [..., hd] fp32, each hd-wide
    row one token's K (after bias and RoPE) or V (after bias) of one kv head -> (codes uint8 [..., hd], e int32 [...],
    image bf16 [..., hd] = code * 2^e), the row quantiser above with the row's largest finite magnitude as amax.  A
    non-finite element takes no part in the row's exponent and becomes the e4m3fn NaN code (sign | 0x7f; NaN in the
    image), never a finite one."""
    x32 = x.detach().float()
    rows = x32.reshape(-1, x32.shape[-1])
    bad = ~torch.isfinite(rows)
    q, e, img = quantize_rows_e4m3(torch.where(bad, torch.zeros_like(rows), rows))
    sign = ((rows.contiguous().view(torch.int32) >> 24) & 0x80).to(torch.uint8)
    q = torch.where(bad, sign | 0x7F, q)
    img = torch.where(bad, torch.full_like(img, float("nan")), img)
    return q.reshape(x32.shape), e.reshape(x32.shape[:-1]), img.reshape(x32.shape)


def pack_codes(q, tile_base=0, tile_stride=1, out=None):
    """q uint8 [N, K] -> the packed order fo_quant_w8 writes ([tile][ceil(K/64)][64 lanes][16 bytes], flat uint8);
    source tile t goes to tile tile_base + t * tile_stride of out (allocated for this weight alone when None)."""
    N, K = q.shape
    nt, KK = (N + 15) // 16, (K + 63) // 64
    p = torch.zeros(nt * 16, KK * 64, dtype=torch.uint8)
    p[:N, :K] = q
    # [tile][row r][step s][half h][lane group g][byte j] -> [tile][s][lane 16 g + r][8 h + j]
    p = p.view(nt, 16, KK, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).reshape(nt, KK * 1024)
    if out is None:
        out = torch.zeros((tile_base + (nt - 1) * tile_stride + 1) * KK * 1024, dtype=torch.uint8)
    out.view(-1, KK * 1024)[tile_base::tile_stride][:nt] = p
    return out


def pack_scales(e, tile_base=0, tile_stride=1, out=None):
    """e int32 [N] -> fp32 2^e at [tile][16] in the same tile order (1 for the rows beyond N)."""
    N = e.shape[0]
    nt = (N + 15) // 16
    s = torch.ones(nt * 16, dtype=torch.float32)
    s[:N] = torch.ldexp(torch.ones(N), e)
    if out is None:
        out = torch.ones((tile_base + (nt - 1) * tile_stride + 1) * 16, dtype=torch.float32)
    out.view(-1, 16)[tile_base::tile_stride][:nt] = s.view(nt, 16)
    return out


# ---------------------------------------------------------------- MXFP4 (mlp_weights="mxfp4"; fo_quant_w4)
#     W'[n, k] = q[n, k] * 2^e[n, k // 32]
# q is an OCP e2m1 code (magnitudes E2M1_GRID as codes 0..7, bit 3 the sign, copied from the weight's sign bit even where
# the magnitude rounds to 0), e one integer per (output row, block of 32 consecutive k): the smallest with
# max|W[n, block]| * 2^-e <= 6, taken from the float's exponent and mantissa (6 = 1.5 * 2^2), at least -125 (so that
# every non-zero q * 2^e is a normal bf16) and 0 for an all-zero block.  W * 2^-e is exact (or an underflow that rounds
# to 0 anyway) and is rounded to the nearest grid point, ties to the even code; nothing saturates, the scaled block
# maximum lies in (3, 6].  q * 2^e has 2 significant bits and is therefore exactly a bf16 value.
E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MX_BLOCK = 32


def block_exponents(w):
    """e[n, k // 32] (int32) of a [N, K] weight, K % 32 == 0."""
    N, K = w.shape
    if K % MX_BLOCK:
        raise ValueError(f"MXFP4 needs K % 32 == 0, got K={K}")
    amax = w.detach().float().abs().view(N, K // MX_BLOCK, MX_BLOCK).amax(dim=2)
    bits = amax.contiguous().view(torch.int32)
    e = (bits >> 23) - 127 - 2 + ((bits & 0x7FFFFF) > 0x400000).to(torch.int32)
    e = e.clamp(min=-125)
    return torch.where(amax > 0, e, torch.zeros_like(e))


def quantize_blocks_e2m1(w):
    """w [N, K] (bf16 or fp32, CPU) -> (q uint8 [N, K] e2m1 codes 0..15, e int32 [N, K // 32], w_dq bf16 [N, K])."""
    w32 = w.detach().float()
    e = block_exponents(w32)
    ek = e.repeat_interleave(MX_BLOCK, dim=1)
    m = torch.ldexp(w32, -ek).abs()
    # nearest grid point, a tie to the even code: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
    code = ((m > 0.25).to(torch.uint8) + (m >= 0.75) + (m > 1.25) + (m >= 1.75) + (m > 2.5) + (m >= 3.5) +
            (m > 5.0)).to(torch.uint8)
    neg = torch.signbit(w32)
    mag = torch.tensor(E2M1_GRID)[code.long()]
    w_dq = torch.ldexp(torch.where(neg, -mag, mag), ek).to(torch.bfloat16)
    return code | (neg.to(torch.uint8) << 3), e, w_dq


def pack_codes_w4(q, tile_base=0, tile_stride=1, out=None):
    """q uint8 [N, K] (codes 0..15) -> the packed order fo_quant_w4 writes ([tile][ceil(K/128)][64 lanes][16 bytes],
    flat uint8, two codes per byte with the lower column in the low nibble); tiles placed as pack_codes does."""
    N, K = q.shape
    nt, KK = (N + 15) // 16, (K + 127) // 128
    p = torch.zeros(nt * 16, KK * 128, dtype=torch.uint8)
    p[:N, :K] = q
    p = p[:, 0::2] | (p[:, 1::2] << 4)          # [row][KK * 64 bytes]: byte c holds columns 2 c, 2 c + 1
    # [tile][row r][step s][k-step j][lane group g][byte b] -> [tile][s][lane 16 g + r][4 j + b]
    p = p.view(nt, 16, KK, 4, 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(nt, KK * 1024)
    if out is None:
        out = torch.zeros((tile_base + (nt - 1) * tile_stride + 1) * KK * 1024, dtype=torch.uint8)
    out.view(-1, KK * 1024)[tile_base::tile_stride][:nt] = p
    return out


def pack_scales_w4(e, tile_base=0, tile_stride=1, out=None):
    """e int32 [N, K // 32] -> E8M0 bytes e + 127 at [tile][ceil(K/128)][16 rows][4] in the same tile order (127 for
    the rows beyond N and the blocks beyond K)."""
    N, KB = e.shape
    nt, KK = (N + 15) // 16, (KB + 3) // 4
    s = torch.full((nt * 16, KK * 4), 127, dtype=torch.uint8)
    s[:N, :KB] = (e + 127).to(torch.uint8)
    s = s.view(nt, 16, KK, 4).permute(0, 2, 1, 3).reshape(nt, KK * 64)
    if out is None:
        out = torch.full(((tile_base + (nt - 1) * tile_stride + 1) * KK * 64,), 127, dtype=torch.uint8)
    out.view(-1, KK * 64)[tile_base::tile_stride][:nt] = s
    return out


# ---------------------------------------------------------------- MXFP6 (mlp_weights="mxfp6"; fo_quant_w6)
#     W'[n, k] = q[n, k] * 2^e[n, k // 32]
# q is an OCP e2m3 code: bit 5 the sign (copied from the weight's sign bit even where the magnitude rounds to 0), bits
# 4..3 the exponent (bias 1), bits 2..0 the mantissa: magnitudes 0, 0.125 .. 0.875 (subnormal), 1 .. 1.875 in steps of
# 0.125, 2 .. 3.75 in steps of 0.25, 4 .. 7.5 in steps of 0.5.  e is one integer per (output row, block of 32 consecutive
# k): the smallest with max|W[n, block]| * 2^-e <= 7.5, taken from the float's exponent and mantissa (7.5 = 1.875 * 2^2),
# at least -123 (so that every non-zero q * 2^e is a normal bf16) and 0 for an all-zero block.  W * 2^-e is exact (or an
# underflow that rounds to 0 anyway) and is rounded to the nearest grid point, ties to the even code; nothing saturates,
# the scaled block maximum lies in (3.75, 7.5].  q * 2^e has 4 significant bits and is therefore exactly a bf16 value.
E2M3_GRID = tuple(m * 0.125 if ex == 0 else (8 + m) * 0.125 * 2.0 ** (ex - 1) for ex in range(4) for m in range(8))


def block_exponents_e2m3(w):
    """e[n, k // 32] (int32) of a [N, K] weight under MXFP6, K % 32 == 0."""
    N, K = w.shape
    if K % MX_BLOCK:
        raise ValueError(f"MXFP6 needs K % 32 == 0, got K={K}")
    amax = w.detach().float().abs().view(N, K // MX_BLOCK, MX_BLOCK).amax(dim=2)
    bits = amax.contiguous().view(torch.int32)
    e = (bits >> 23) - 127 - 2 + ((bits & 0x7FFFFF) > 0x700000).to(torch.int32)
    e = e.clamp(min=-123)
    return torch.where(amax > 0, e, torch.zeros_like(e))


def quantize_blocks_e2m3(w):
    """w [N, K] (bf16 or fp32, CPU) -> (q uint8 [N, K] e2m3 codes 0..63, e int32 [N, K // 32], w_dq bf16 [N, K])."""
    w32 = w.detach().float()
    e = block_exponents_e2m3(w32)
    ek = e.repeat_interleave(MX_BLOCK, dim=1)
    m = torch.ldexp(w32, -ek).abs()
    # the grid's step is 1/8 below 2, 1/4 below 4 and 1/2 up to 7.5; torch.round is nearest with ties to the even
    # integer, which is the even code (the offsets 0, 8, 16 are even): 0.0625 -> 0, 0.1875 -> 0.25, 7.25 -> 7.0
    code = torch.where(m < 2, torch.round(m * 8), torch.where(m < 4, 8 + torch.round(m * 4), 16 + torch.round(m * 2)))
    code = code.to(torch.uint8)
    neg = torch.signbit(w32)
    mag = torch.tensor(E2M3_GRID)[code.long()]
    w_dq = torch.ldexp(torch.where(neg, -mag, mag), ek).to(torch.bfloat16)
    return code | (neg.to(torch.uint8) << 5), e, w_dq


W6_STEP = 1536      # bytes of one code step of one packed tile: 2 planes x 64 lanes x 12


def pack_codes_w6(q, tile_base=0, tile_stride=1, out=None):
    """q uint8 [N, K] (codes 0..63) -> the packed order fo_quant_w6 writes ([tile][ceil(K/128)][2 planes][64 lanes]
    [12 bytes], flat uint8): lane 16 g + r of code step s holds columns 128 s + 32 g .. + 31 of row r, column j at bits
    [6 j, 6 j + 6) of its 24 bytes (little-endian), the first 12 bytes in plane 0 and the last 12 in plane 1; tiles
    placed as pack_codes does."""
    N, K = q.shape
    nt, KK = (N + 15) // 16, (K + 127) // 128
    p = torch.zeros(nt * 16, KK * 128, dtype=torch.int32)
    p[:N, :K] = q
    c = p.view(nt * 16, KK * 32, 4)             # four codes -> three bytes
    b = torch.stack((c[..., 0] | ((c[..., 1] & 3) << 6), (c[..., 1] >> 2) | ((c[..., 2] & 15) << 4),
                     (c[..., 2] >> 4) | (c[..., 3] << 2)), dim=-1).to(torch.uint8)
    # [tile][row r][step s][lane group g][plane p][byte b] -> [tile][s][p][lane 16 g + r][b]
    b = b.view(nt, 16, KK, 4, 2, 12).permute(0, 2, 4, 3, 1, 5).reshape(nt, KK * W6_STEP)
    if out is None:
        out = torch.zeros((tile_base + (nt - 1) * tile_stride + 1) * KK * W6_STEP, dtype=torch.uint8)
    out.view(-1, KK * W6_STEP)[tile_base::tile_stride][:nt] = b
    return out


def pack_scales_w6(e, tile_base=0, tile_stride=1, out=None):
    """e int32 [N, K // 32] -> E8M0 bytes e + 127 at [tile][ceil(K/128)][16 rows][4]: pack_scales_w4's order (byte g of
    row r's dword is lane (r, g)'s scale)."""
    return pack_scales_w4(e, tile_base, tile_stride, out)


# ---------------------------------------------------------------- the fused q|k|v weight (attn_weights; hd % 32 == 0)
# The rope-paired tile order of PackedLinear(rope_hd=hd) and of fo_gemm_w8_qkv_rope / fo_gemm_w4_qkv_rope: for head h
# and half p in {0, 1}, the hd/2 rows from h * hd + p * hd/2 go to packed tiles h * (hd/16) + p, + 2, ..., so adjacent
# packed tiles (2P, 2P + 1) hold columns (i, i + hd/2) of one head.  One pack_* call per (head, half).
def _rope_pack(pack, x, hd, out):
    N = x.shape[0]
    if hd % 32 or N % hd:
        raise ValueError(f"rope packing needs hd % 32 == 0 and N % hd == 0 (N={N}, hd={hd})")
    half = hd // 2
    for h in range(N // hd):
        for p in (0, 1):
            r0 = h * hd + p * half
            out = pack(x[r0:r0 + half], tile_base=h * (hd // 16) + p, tile_stride=2, out=out)
    return out


def pack_codes_rope(q, hd):
    """q uint8 [N, K] e4m3fn codes of a fused q|k|v weight -> fo_quant_w8's packed codes in the rope-paired order."""
    N, K = q.shape
    return _rope_pack(pack_codes, q, hd, torch.zeros(N // 16 * ((K + 63) // 64) * 1024, dtype=torch.uint8))


def pack_scales_rope(e, hd):
    """e int32 [N] -> fp32 2^e at [tile][16] in the rope-paired order."""
    return _rope_pack(pack_scales, e, hd, torch.ones(e.shape[0], dtype=torch.float32))


def pack_codes_rope_w4(q, hd):
    """q uint8 [N, K] e2m1 codes of a fused q|k|v weight -> fo_quant_w4's packed codes in the rope-paired order."""
    N, K = q.shape
    return _rope_pack(pack_codes_w4, q, hd, torch.zeros(N // 16 * ((K + 127) // 128) * 1024, dtype=torch.uint8))


def pack_scales_rope_w4(e, hd):
    """e int32 [N, K // 32] -> E8M0 bytes at [tile][ceil(K/128)][16 rows][4] in the rope-paired order."""
    N, KB = e.shape
    return _rope_pack(pack_scales_w4, e, hd, torch.full((N // 16 * ((KB + 3) // 4) * 64,), 127, dtype=torch.uint8))
