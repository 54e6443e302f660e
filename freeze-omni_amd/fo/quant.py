"""CPU reference of the weight-only FP8 quantiser (include/fo_hip.h fo_quant_w8): the definition of the
`mlp_weights="fp8"` model, used by tests and docs.  torch on the host only; the engine quantises on the device.

    W'[n, k] = q[n, k] * 2^e[n]

q is an OCP e4m3fn code (gfx950's format), e[n] one integer per output row: the smallest with
max|W[n, :]| * 2^-e[n] <= 448, taken from the float's exponent and mantissa (448 = 1.75 * 2^8), 0 for an all-zero row.
W * 2^-e is exact, so the rounding to e4m3fn (nearest-even) never saturates; q * 2^e has at most 4 significant bits and
is therefore exactly a bf16 value.
"""
import torch

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
