// Weight-only MXFP6 (OCP e2m3 codes, one power-of-two scale per 32 elements) GEMMs for the Qwen2 MLP at <= 16 rows
// (fo_gemm_w6; fo_gemm_w6_head for the lm_head: k_w6_xs's plain form) and at 17..64 rows (fo_gemm_w6_rows: k_w6_rows,
// then k_w8_rows_merge of fo_gemm_wq.h where K is split), and their quantiser.
//
//   W'[n, k] = q[n, k] * 2^e[n, k / 32]   q an e2m3 code (1 sign, 2 exponent bits of bias 1, 3 mantissa bits: 0,
//                                         0.125 .. 0.875, 1 .. 1.875, 2 .. 3.75, 4 .. 7.5), e one integer per (output
//                                         row, block of 32 columns), stored as the E8M0 byte e + 127
//   Y[M, N]  = epilogue( X[M, K] (fp32, split into bf16 hi + lo) . W'^T )
//
// An e2m3 value has 4 significant bits, so q * 2^e is exactly a bf16 value: W' has an exact bf16 image, which the
// engine keeps packed for the bf16 kernels and runs wherever the codes are not streamed.  The kernels here stream the
// codes -- 6.25 bits per weight with the scales -- decode a lane's 32 codes to bf16 with the block scale applied in one
// instruction (v_cvt_scalef32_pk32_bf16_fp6: exact) and run the same bf16 MFMAs as fo_gemm_w4.hip, with its epilogue
// (fo_gemm_wq.h, no column scale).  Results are deterministic in every form.
//
// Code layout (include/fo_hip.h): [tile][K128][2 planes][64 lanes][12 bytes].  Lane 16 g + r of code step s holds the
// 32 consecutive columns 128 s + 32 g .. + 31 of row r -- one MX block, one scale -- as 32 six-bit codes, column j at
// bits [6 j, 6 j + 6) of the lane's 192-bit field; plane p is dwords 3 p .. 3 p + 2 of that field (columns 16 p .. + 15),
// so each of the two 12-byte loads of a wave reads 768 contiguous bytes.  The lane's values 8 t .. 8 t + 7 are its B
// fragment of MFMA sub-step t, so its A fragment there is X[row][128 s + 32 g + 8 t .. + 7]: not fo_gemm_w4's k order,
// and legal because A and B use the same assignment.  K is padded to a multiple of 128 with zero codes; scale bytes
// [tile][K128][16 rows][4] as MXFP4's, lane (r, g) using byte g of row r's dword.
#include <stdlib.h>

#include <atomic>

#include "fo_gemm_wq.h"

namespace {

typedef __attribute__((ext_vector_type(3))) unsigned u32x3;
typedef __attribute__((ext_vector_type(6))) unsigned u32x6;
typedef __attribute__((ext_vector_type(32))) __bf16 bf16x32;

constexpr int W6_STEP = 1536;   // bytes of one code step of one tile (64 lanes x 24)

struct W6Q {
  u32x3 p0, p1;   // the lane's two planes: codes 0..15, 16..31
};
struct W6Frag {
  bf16x8 f[4];    // the B fragments of the four MFMA sub-steps
};

// 32 e2m3 codes times 2^(sb - 127) -> 32 bf16, one instruction
__device__ __forceinline__ W6Frag dec6(const W6Q& q, unsigned sb) {
  const u32x6 v = {q.p0[0], q.p0[1], q.p0[2], q.p1[0], q.p1[1], q.p1[2]};
  const bf16x32 w = __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(v, __uint_as_float(sb << 23));
  return __builtin_bit_cast(W6Frag, w);
}

// The two descriptors cover exactly the codes (ntiles * KK * 1536) and the scale bytes (ntiles * KK * 64): a tile at or
// past ntiles is out of range and loads zero codes under a zero scale byte (2^-127 times 0)
struct W6Srd {
  __amdgpu_buffer_rsrc_t q, s;
};
__device__ __forceinline__ W6Srd w6_srd(const W8Args& a) {
  return W6Srd{rsrc_of(a.Q, a.ntiles * a.KK * W6_STEP), rsrc_of(a.scale, a.ntiles * a.KK * 64)};
}
__device__ __forceinline__ W6Q w6_codes(const W6Srd& d, int lane, int step) {   // step = tile * KK + code step
  W6Q q;
  q.p0 = __builtin_bit_cast(u32x3, __builtin_amdgcn_raw_buffer_load_b96(d.q, lane * 12, step * W6_STEP, 2));
  q.p1 = __builtin_bit_cast(u32x3, __builtin_amdgcn_raw_buffer_load_b96(d.q, 768 + lane * 12, step * W6_STEP, 2));
  return q;
}
// the lane's scale byte: byte lane >> 4 of row lane & 15's dword (w6_scale_dword: that dword as loaded, for a kernel
// that keeps the load in flight and takes the byte where it decodes)
__device__ __forceinline__ unsigned w6_scale_dword(const W6Srd& d, int lane, int step) {
  return __builtin_amdgcn_raw_buffer_load_b32(d.s, (lane & 15) * 4, step * 64, 0);
}
__device__ __forceinline__ unsigned w6_scale_byte(unsigned dword, int lane) { return (dword >> (8 * (lane >> 4))) & 0xffu; }
__device__ __forceinline__ unsigned w6_scale(const W6Srd& d, int lane, int step) {
  return w6_scale_byte(w6_scale_dword(d, lane, step), lane);
}

// A 4 x 4 transpose across the four lane groups of a wave (lanes r, r + 16, r + 32, r + 48), one dword per (register,
// lane): afterwards lane group g holds in a[t] what lane group t held in a[g].  Two v_permlane32_swap (the 2 x 2 blocks)
// then two v_permlane16_swap (inside the blocks); every lane of the wave must be active.
__device__ __forceinline__ void xpose4(unsigned (&a)[4]) {
  const auto s02 = __builtin_amdgcn_permlane32_swap(a[0], a[2], false, false);
  const auto s13 = __builtin_amdgcn_permlane32_swap(a[1], a[3], false, false);
  const auto t01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
  const auto t23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
  a[0] = t01[0];
  a[1] = t01[1];
  a[2] = t23[0];
  a[3] = t23[1];
}
__device__ __forceinline__ void xpose4(bf16x8 (&f)[4]) {
  u32x4 v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = __builtin_bit_cast(u32x4, f[j]);
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    unsigned a[4] = {v[0][d], v[1][d], v[2][d], v[3][d]};
    xpose4(a);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j][d] = a[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) f[j] = __builtin_bit_cast(bf16x8, v[j]);
}

// acc[t] = X[rows 0..16, code steps [kb, ke)] . (packed tile tile0 + t)^T for t < NT: U code steps in flight, each X
// fragment loaded and split once for the NT tiles.  xp: the lane's row at column 8 (lane >> 4).  X is loaded as the
// bf16 and MXFP4 kernels load it -- load j of lane (r, g') reads columns 128 kk + 32 j + 8 g' .. + 7, so the four lane
// groups of a row share one 128-byte line (the layout's own assignment, 32 consecutive columns per lane, touches four
// times as many lines per load and cost the down projection 5 us at 16 rows) -- and the split fragments are transposed
// across the lane groups (xpose4) into the layout's assignment: lane (r, g) sub-step t = columns 128 kk + 32 g + 8 t.
// A 32-column block at or past K (K % 128 != 0: load j of the last code step, wave-uniform) reads no X and holds
// zeros, which the transpose hands to lane group j as its zero A fragments; the other groups of the same MFMAs are live.
template <int NT, int U>
__device__ __forceinline__ void w6_accumulate(const W8Args& a, const W6Srd& d, const float* xp, int lane, int tile0,
                                              int kb, int ke, f32x4 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = kb; k0 < ke; k0 += U) {
    W6Q q[U][NT];
    unsigned sc[U][NT];
    float4 x[U][8];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int kk = k0 + i;
      if (kk < ke) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          q[i][t] = w6_codes(d, lane, (tile0 + t) * a.KK + kk);
          sc[i][t] = w6_scale(d, lane, (tile0 + t) * a.KK + kk);
        }
        const float* p = xp + (size_t)kk * 128;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool live = kk * 128 + 32 * j < a.K;
          x[i][2 * j] = live ? reinterpret_cast<const float4*>(p + 32 * j)[0] : float4{0.f, 0.f, 0.f, 0.f};
          x[i][2 * j + 1] = live ? reinterpret_cast<const float4*>(p + 32 * j)[1] : float4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int kk = k0 + i;
      if (kk < ke) {
        bf16x8 hi[4], lo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) split8(x[i][2 * j], x[i][2 * j + 1], hi[j], lo[j]);
        xpose4(hi);
        xpose4(lo);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const W6Frag w = dec6(q[i][t], sc[i][t]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi[j], w.f[j], acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo[j], w.f[j], acc[t], 0, 0, 0);
          }
        }
      }
    }
  }
}

// ---- general form: workgroup u = output tile u (SW: the (gate, up) pair 2u, 2u + 1); wave w takes the code steps
// [KK w / NW, KK (w + 1) / NW), one (per tile) in flight
template <int NW, bool SW>
__global__ __launch_bounds__(NW * 64) void k_w6(W8Args a) {
  constexpr int T = SW ? 2 : 1;
  __shared__ float part[NW][T][16][17];
  __shared__ float rstd_s[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = blockIdx.x;
  const W6Srd d = w6_srd(a);
  const int kb = (int)((long)a.KK * wave / NW), ke = (int)((long)a.KK * (wave + 1) / NW);
  const int row = min(lane & 15, a.M - 1);
  const float* xp = a.X + (size_t)row * a.ldx + 8 * (lane >> 4);
  if (a.rstats) w8_rstd<NW>(a, rstd_s, wave, lane);
  f32x4 acc[T];
  w6_accumulate<T, 1>(a, d, xp, lane, T * u, kb, ke, acc);
#pragma unroll
  for (int t = 0; t < T; ++t) w8_store_tile(part[wave][t], acc[t], lane);
  __syncthreads();
  const int e = threadIdx.x;
  if (e < 256) {
    const int rr = e >> 4, c = e & 15;
    float x1 = 0.f, x2 = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      x1 += part[w][0][rr][c];
      if constexpr (SW) x2 += part[w][1][rr][c];
    }
    w8_epilogue<SW, false>(a, u, gridDim.x, rr, c, x1, x2, rstd_s);
  }
}

// ---- long-K plain form, as k_w4_sk: workgroup (tg, sp) = tiles NT tg .. + NT over the sp-th of S slices of the code
// steps, the slice split over the waves as in k_w6.  ws: S slabs of [16][groups * NT * 16] partial sums; counters: one
// zeroed ticket per tile group, left zeroed.  The hand-off is fo_common.h's (st_wt / ld_sc1): no fences, no waiting;
// the last split to arrive sums every split's partial in split order.
template <int NW, int NT>
__global__ __launch_bounds__(NW * 64) void k_w6_sk(W8Args a, int S, float* ws, int* counters) {
  __shared__ float part[NW][NT][16][17];
  __shared__ float red[NT][16][17];
  __shared__ float rstd_s[16];
  __shared__ int last_s;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tg = blockIdx.x, sp = blockIdx.y;
  const W6Srd d = w6_srd(a);
  const int k_lo = (int)((long)a.KK * sp / S), k_n = (int)((long)a.KK * (sp + 1) / S) - k_lo;
  const int kb = k_lo + (int)((long)k_n * wave / NW), ke = k_lo + (int)((long)k_n * (wave + 1) / NW);
  const int row = min(lane & 15, a.M - 1);
  const float* xp = a.X + (size_t)row * a.ldx + 8 * (lane >> 4);
  if (a.rstats) w8_rstd<NW>(a, rstd_s, wave, lane);
  f32x4 acc[NT];
  w6_accumulate<NT, 1>(a, d, xp, lane, NT * tg, kb, ke, acc);
#pragma unroll
  for (int t = 0; t < NT; ++t) w8_store_tile(part[wave][t], acc[t], lane);
  __syncthreads();
  constexpr int NE = NT * 256, NTH = NW * 64;
  for (int e = threadIdx.x; e < NE; e += NTH) {
    const int t = e >> 8, rr = (e >> 4) & 15, c = e & 15;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += part[w][t][rr][c];
    red[t][rr][c] = v;
  }
  if (S > 1) {
    const int Ncols = gridDim.x * NT * 16;
    const size_t sl = (size_t)16 * Ncols;
    float* slab = ws + (size_t)sp * sl;
    for (int e = threadIdx.x; e < NE; e += NTH) {   // (each thread stores the elements it just summed)
      const int t = e >> 8, rr = (e >> 4) & 15, c = e & 15;
      st_wt(slab + (size_t)rr * Ncols + (tg * NT + t) * 16 + c, red[t][rr][c]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      int* tk = counters + tg;
      const int old = __hip_atomic_fetch_add(tk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last_s = old == S - 1;
      if (old == S - 1) __hip_atomic_store(tk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last_s) return;
    const __amdgpu_buffer_rsrc_t rws = rsrc_of(ws);
    for (int e = threadIdx.x; e < NE; e += NTH) {
      const int t = e >> 8, rr = (e >> 4) & 15, c = e & 15;
      const size_t o = (size_t)rr * Ncols + (tg * NT + t) * 16 + c;
      const float own = red[t][rr][c];
      float v = 0.f;
      for (int q0 = 0; q0 < S; ++q0) v += q0 != sp ? ld_sc1(rws, q0 * sl + o) : own;
      red[t][rr][c] = v;
    }
  }
  __syncthreads();
  const int units = (a.N + 15) / 16;
  if (threadIdx.x < 256) {
    const int rr = threadIdx.x >> 4, c = threadIdx.x & 15;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (tg * NT + t < units) w8_epilogue<false, false>(a, tg * NT + t, units, rr, c, red[t][rr][c], 0.f, rstd_s);
  }
}

// ---- X-stationary persistent form, as k_w4_xs: the SwiGLU pair, K = NW * KPW * 128 (3584 = 28 code steps).  X hi in
// registers, lo in LDS, units dealt evenly to at most one workgroup per CU, the next unit's codes and scales issued
// before the current one is reduced, a fixed-order cross-wave reduction.
// SW = false (fo_gemm_w6_head): the plain form.  A unit is two adjacent plain tiles 2u, 2u + 1 (the second of an odd
// count's last unit lies past both descriptors: zero codes under a zero scale byte, never stored), each with the plain
// epilogue: the store, no residual, no statistics (NW * 64 >= 512: a tile per 256 threads).
template <int NW, int KPW, bool SW = true>
__global__ __launch_bounds__(NW * 64) void k_w6_xs(W8Args a, int units) {
  static_assert(SW || NW >= 8, "k_w6_xs: the plain epilogue takes 512 threads");
  __shared__ bf16x8 xlo[NW][4 * KPW][64];
  __shared__ float part[NW][2][16][17];
  __shared__ float rstd_s[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int KK = NW * KPW;
  const int ub = (int)((long)units * blockIdx.x / gridDim.x);
  const int ue = (int)((long)units * (blockIdx.x + 1) / gridDim.x);
  const W6Srd d = w6_srd(a);
  W6Q q0[KPW], q1[KPW];
  unsigned s0[KPW], s1[KPW];
  auto issue = [&](W6Q (&q)[KPW], unsigned (&s)[KPW], int tile) {
#pragma unroll
    for (int j = 0; j < KPW; ++j) {
      q[j] = w6_codes(d, lane, tile * KK + wave * KPW + j);
      s[j] = w6_scale(d, lane, tile * KK + wave * KPW + j);
    }
  };
  issue(q0, s0, ub < ue ? 2 * ub : a.ntiles);
  issue(q1, s1, ub < ue ? 2 * ub + 1 : a.ntiles);
  // X slice (hi in registers, lo in LDS); rows >= M clamp to the last row (computed, never stored)
  bf16x8 xh[4 * KPW];
  {
    const int row = min(lane & 15, a.M - 1);
    const float* xp = a.X + (size_t)row * a.ldx + 32 * (lane >> 4) + (size_t)wave * KPW * 128;
#pragma unroll
    for (int j = 0; j < 4 * KPW; ++j) {
      const float4* p = reinterpret_cast<const float4*>(xp + (j >> 2) * 128 + (j & 3) * 8);
      bf16x8 lo;
      split8(p[0], p[1], xh[j], lo);
      xlo[wave][j][lane] = lo;
    }
  }
  if constexpr (SW) {
    if (a.rstats) w8_rstd<NW>(a, rstd_s, wave, lane);
  }
  auto compute = [&](W6Q (&q)[KPW], unsigned (&s)[KPW]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // (the lo fragments are re-read from LDS per tile: an opaque lane index keeps the compiler from hoisting the
    // loop-invariant reads into 4 KPW more live registers, which spilled at 14 waves)
    int ln = lane;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int j = 0; j < KPW; ++j) {
      const W6Frag w = dec6(q[j], s[j]);
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[4 * j + h], w.f[h], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xlo[wave][4 * j + h][ln], w.f[h], acc, 0, 0, 0);
      }
    }
    return acc;
  };
  for (int u = ub; u < ue; ++u) {
    // the next unit's codes are issued unconditionally; past the last unit they address tile `ntiles`, beyond the
    // descriptors' range, which the hardware drops without touching memory
    const int nxt = u + 1 < ue ? 2 * (u + 1) : a.ntiles;
    const f32x4 c0 = compute(q0, s0);
    issue(q0, s0, nxt);
    const f32x4 c1 = compute(q1, s1);
    issue(q1, s1, nxt + (u + 1 < ue ? 1 : 0));
    __syncthreads();  // the previous unit's epilogue has read part[]
    w8_store_tile(part[wave][0], c0, lane);
    w8_store_tile(part[wave][1], c1, lane);
    __syncthreads();
    const int e = threadIdx.x;
    if constexpr (SW) {
      if (e < 256) {
        const int rr = e >> 4, c = e & 15;
        float x1 = 0.f, x2 = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          x1 += part[w][0][rr][c];
          x2 += part[w][1][rr][c];
        }
        w8_epilogue<true, false>(a, u, 0, rr, c, x1, x2, rstd_s);
      }
    } else if (e < 512) {
      const int t = e >> 8, rr = (e >> 4) & 15, c = e & 15;
      float x1 = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) x1 += part[w][t][rr][c];
      if (2 * u + t < a.ntiles) w8_epilogue<false, false>(a, 2 * u + t, 0, rr, c, x1, 0.f, rstd_s);
    }
  }
}

// ---- 17..64 rows (RB = 2..4 row blocks of 16; fo_gemm_w6_rows): k_w4_rows's design (fo_gemm_w4.hip) on this file's
// code layout.  Workgroup (g, sp): the sp-th of S slices of the code steps for units [ub, ue) of column group g; a unit
// is a packed tile pair (the (gate, up) pair, or two adjacent plain tiles: the second of an odd count's last pair lies
// past both descriptors and loads zero codes under a zero scale byte).  Wave w owns KPW code steps of the slice.  Their
// X fragments of all RB row blocks follow the layout's assignment -- lane (r, g), sub-step t of code step s:
// X[row][128 s + 32 g + 8 t .. + 7], k_w6_xs's direct load -- and are split once (hi in VGPRs, lo in the wave's LDS
// region).  A lane whose 32-column block lies at or past K (K % 128 = 32, 64 or 96, the last code step: a condition
// per lane group, not per wave) reads no X -- X may end at the last row's column K -- and holds zero fragments.  Per
// (tile, code step) two 12-byte plane loads and the scale dword; one dec6 gives the 4 B fragments that feed
// RB x (hi, lo) MFMAs each.  The next two units' codes and scales are in flight meanwhile.  Per unit the NW partial
// tiles are summed through LDS in wave order (both tiles in one round where the LDS allows).  S == 1: the epilogue
// follows.  S > 1: the sums are stored as split sp's slab of `ws` ([S][RB * 16][ntiles * 16] floats) and
// k_w8_rows_merge (fo_gemm_wq.h, unscaled), the next launch, sums the slabs in split order and runs the epilogue.
template <int NW, int KPW, int RB, bool SW>
__global__ __launch_bounds__(NW * 64) void k_w6_rows(W8Args a, int S, int per, float* ws) {
  constexpr int ROWS = RB * 16, NTH = NW * 64, NE = ROWS * 16, EPT = (NE + NTH - 1) / NTH;
  constexpr int PT = (NW * RB * 4 * KPW * 1024 + NW * 2 * ROWS * 17 * 4 + 512 <= 160 * 1024) ? 2 : 1;
  __shared__ bf16x8 xlo[NW][RB][4 * KPW][64];
  __shared__ float part[NW][PT][ROWS][17];
  __shared__ float rstd_s[ROWS];
  // (the wave index through readfirstlane: the code steps' offsets are then scalars the buffer loads take as they are)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int G = gridDim.x, g = blockIdx.x, sp = blockIdx.y;
  const int units = (a.ntiles + 1) >> 1, tiles = (a.N + 15) / 16;   // (tiles: output tiles, the statistics' groups)
  const int ub = (int)((long)units * g / G), ue = (int)((long)units * (g + 1) / G);
  const W6Srd d = w6_srd(a);   // (exactly the codes and the scale bytes)
  // this wave's code steps: [k0, k0 + nj) inside the slice [sp * per, (sp + 1) * per) and inside KK (wave-uniform)
  const int k0 = sp * per + wave * KPW;
  const int nj = max(0, min(KPW, min(a.KK, (sp + 1) * per) - k0));
  W6Q q[2][2][KPW];
  unsigned sc[2][2][KPW];   // (the scale dwords as loaded: the lane's byte is taken where they are decoded)
  auto issue = [&](W6Q (&qq)[2][KPW], unsigned (&ss)[2][KPW], int u) {   // u >= ue: no load issued
    if (u < ue) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < KPW; ++j)
          if (j < nj) {
            qq[t][j] = w6_codes(d, lane, (2 * u + t) * a.KK + k0 + j);
            ss[t][j] = w6_scale_dword(d, lane, (2 * u + t) * a.KK + k0 + j);
          }
    }
  };
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < KPW; ++j) {   // code steps past the slice: zero codes under a zero scale byte
        q[b][t][j].p0 = q[b][t][j].p1 = u32x3{0u, 0u, 0u};
        sc[b][t][j] = 0u;
      }
  issue(q[0], sc[0], ub);
  issue(q[1], sc[1], ub + 1);
  bf16x8 zero;
#pragma unroll
  for (int i = 0; i < 8; ++i) zero[i] = (__bf16)0.f;
  bf16x8 xh[RB][4 * KPW];
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const int row = min(r * 16 + (lane & 15), a.M - 1);   // rows >= M: computed, never stored or summed
    const float* xp = a.X + (size_t)row * a.ldx + 32 * (lane >> 4);
#pragma unroll
    for (int j = 0; j < 4 * KPW; ++j) {
      bf16x8 hi = zero, lo = zero;
      const int blk = (k0 + (j >> 2)) * 128 + 32 * (lane >> 4);   // the lane's block of this code step: in K or past it
      if ((j >> 2) < nj && blk < a.K) {
        const float4* p = reinterpret_cast<const float4*>(xp + (size_t)(k0 + (j >> 2)) * 128 + (j & 3) * 8);
        split8(p[0], p[1], hi, lo);
      }
      xh[r][j] = hi;
      xlo[wave][r][j][lane] = lo;
    }
  }
  if (S == 1) {   // the consumer's rstd of every row (rows >= M from the clamped row)
    if (a.rstats) w8_rstd<NW>(a, rstd_s, wave, lane, 0, ROWS);
    __syncthreads();
  }
  const int Ncols = a.ntiles * 16;
  float* slab = ws + (size_t)sp * ROWS * Ncols;
  auto unit = [&](W6Q (&qq)[2][KPW], unsigned (&ss)[2][KPW], int u) {
    float v[2][EPT];
    // (the lo fragments are re-read from LDS per unit, as in k_w6_xs: an opaque lane index keeps the compiler from
    // hoisting the loop-invariant reads into RB * 4 KPW more live registers, which spilled at 2 row blocks)
    int ln = lane;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int t0 = 0; t0 < 2; t0 += PT) {
      f32x4 acc[PT][RB];
#pragma unroll
      for (int p = 0; p < PT; ++p) {
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[p][r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KPW; ++j) {
          const W6Frag w = dec6(qq[t0 + p][j], w6_scale_byte(ss[t0 + p][j], lane));
#pragma unroll
          for (int h = 0; h < 4; ++h)
#pragma unroll
            for (int r = 0; r < RB; ++r) {
              acc[p][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[r][4 * j + h], w.f[h], acc[p][r], 0, 0, 0);
              acc[p][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xlo[wave][r][4 * j + h][ln], w.f[h], acc[p][r], 0, 0, 0);
            }
        }
      }
      if (t0 + PT == 2) issue(qq, ss, u + 2);   // (the unit's codes are decoded: its buffer takes the unit after next)
      __syncthreads();  // the previous reduction has read part[]
#pragma unroll
      for (int p = 0; p < PT; ++p)
#pragma unroll
        for (int r = 0; r < RB; ++r) w8_store_tile(part[wave][p], acc[p][r], lane, r * 16);
      __syncthreads();
#pragma unroll
      for (int p = 0; p < PT; ++p)
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
          const int e = threadIdx.x + i * NTH;
          float s = 0.f;
          if (e < NE) {
#pragma unroll
            for (int w = 0; w < NW; ++w) s += part[w][p][e >> 4][e & 15];
            if (S > 1 && 2 * u + t0 + p < a.ntiles)
              slab[(size_t)(e >> 4) * Ncols + (2 * u + t0 + p) * 16 + (e & 15)] = s;
          }
          v[t0 + p][i] = s;
        }
    }
    if (S == 1) {
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        const int e = threadIdx.x + i * NTH;   // (NTH % 16 == 0: a row's 16 columns are one 16-lane row of a wave)
        const int rr = e < NE ? e >> 4 : ROWS, c = e & 15;
        if constexpr (SW) {
          w8_epilogue<true, false>(a, u, tiles, rr, c, v[0][i], v[1][i], rstd_s);
        } else {
          w8_epilogue<false, false>(a, 2 * u, tiles, rr, c, v[0][i], 0.f, rstd_s);
          if (2 * u + 1 < a.ntiles) w8_epilogue<false, false>(a, 2 * u + 1, tiles, rr, c, v[1][i], 0.f, rstd_s);
        }
      }
    }
  };
  for (int u = ub; u < ue; u += 2) {   // (workgroup-uniform: every wave reaches unit's barriers)
    unit(q[0], sc[0], u);
    if (u + 1 < ue) unit(q[1], sc[1], u + 1);
  }
}

// ---- quantiser.  One workgroup per source row n, one 32-column block per thread and pass: the block's amax, e from
// its exponent and mantissa (the smallest integer with amax * 2^-e <= 7.5 = 1.875 * 2^2, at least -123 so that every
// non-zero q * 2^e is a normal bf16; 0 for an all-zero block), W * 2^-e (exact, or an underflow that rounds to 0 anyway)
// rounded to the nearest e2m3 magnitude, ties to the even code, the sign bit copied; then the block's six dwords to the
// two planes of lane 16 g + (n & 15) (g = the block's index in its code step), its scale byte, and the 32 dequantised
// bf16 values to wdq.  Columns K .. 128 KK and rows N .. 16 ceil(N / 16) get zero codes and scale byte 127.
__device__ __forceinline__ unsigned e2m3_code(float v) {
  // the grid's step is 1/8 below 2, 1/4 below 4, 1/2 up to 7.5: rintf rounds to nearest, ties to the even integer,
  // which is the even code (the three offsets are even)
  const float m = fabsf(v);
  const unsigned c = m < 2.f ? (unsigned)rintf(m * 8.f) : (m < 4.f ? 8u + (unsigned)rintf(m * 4.f) : 16u + (unsigned)rintf(m * 2.f));
  return c | ((__float_as_uint(v) >> 26) & 32u);
}

__global__ __launch_bounds__(256) void k_quant_w6(const void* W, int src_bf16, int N, int K, int ldw, unsigned char* q,
                                                  unsigned char* scale, bf16_t* wdq, int KK, int tile_base,
                                                  int tile_stride) {
  const int n = blockIdx.x;
  auto at = [&](int k) {
    return src_bf16 ? bf2f(reinterpret_cast<const bf16_t*>(W)[(size_t)n * ldw + k])
                    : reinterpret_cast<const float*>(W)[(size_t)n * ldw + k];
  };
  const size_t dt = (size_t)tile_base + (size_t)(n >> 4) * tile_stride;
  for (int b = threadIdx.x; b < KK * 4; b += 256) {   // block b: columns 32 b .. + 32, lane group b & 3 of code step b >> 2
    const bool live = n < N && 32 * b < K;   // (K % 32 == 0: a block is inside K or past it)
    float v[32];
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      v[j] = live ? at(32 * b + j) : 0.f;
      amax = fmaxf(amax, fabsf(v[j]));
    }
    int e = 0;
    if (amax > 0.f) {
      const unsigned bits = __float_as_uint(amax);
      e = (int)(bits >> 23) - 127 - 2 + ((bits & 0x7fffffu) > 0x700000u ? 1 : 0);
      e = max(e, -123);
    }
    const float s = __uint_as_float((unsigned)(e + 127) << 23), inv = __uint_as_float((unsigned)(127 - e) << 23);
    const int kk = b >> 2, g = b & 3;
    scale[((dt * KK + kk) * 16 + (n & 15)) * 4 + g] = (unsigned char)(e + 127);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      unsigned dw[3] = {0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const unsigned c = e2m3_code(v[16 * p + j] * inv);
        const int bit = 6 * j;
        dw[bit >> 5] |= c << (bit & 31);
        if ((bit & 31) > 26) dw[(bit >> 5) + 1] |= c >> (32 - (bit & 31));
        if (wdq && live) {
          const unsigned ex = (c >> 3) & 3u, mn = c & 7u;
          const float mag = ex ? 0.125f * (float)((8u + mn) << (ex - 1u)) : 0.125f * (float)mn;
          wdq[(size_t)n * K + 32 * b + 16 * p + j] =
              f2bf(__uint_as_float(__float_as_uint(mag * s) | ((c & 32u) << 26)));
        }
      }
      unsigned* o = reinterpret_cast<unsigned*>(q + ((dt * KK + kk) * 2 + p) * 768 + (16 * g + (n & 15)) * 12);
      o[0] = dw[0];
      o[1] = dw[1];
      o[2] = dw[2];
    }
  }
}

int g_cus = 0;
int w6_cus() {
  if (!g_cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    g_cus = n;
  }
  return g_cus;
}

// the launch counters (fo_gemm_w6_counts): fo_gemm_w6's general, xs and sk forms, and fo_gemm_w6_head; and the calls of
// fo_gemm_w6_rows (fo_gemm_w6_rows_count)
std::atomic<long long> g_w6_launches[4];
std::atomic<long long> g_w6_rows_calls;

// What the GEMM entries share: the checks of everything but the workspace (all before the entry's first HIP call),
// then W8Args (with KK) and the output tile count.  `fn` is the entry's name, [m_lo, m_hi] its row band and `serves`
// what its refusal says of the band.
constexpr const char* W6_SERVES_16 = "the MXFP6 stream serves M <= 16 (more rows run the bf16 image)";
int w6_args(const char* fn, int m_lo, int m_hi, const char* serves, const float* X, int ldx, int M, int K, const void* Q,
            const void* scale, int ntiles, int N, int swiglu, float* Y, int ldy, int residual, const float* rstats,
            int rgroups, float eps, float* sout, const float* gnext, float* yg, W8Args& a, int& units) {
  FO_REQUIRE(M > 0 && N > 0 && K > 0, "%s: bad shape M=%d N=%d K=%d", fn, M, N, K);
  FO_REQUIRE(M >= m_lo && M <= m_hi, "%s: M=%d rows, %s", fn, M, serves);
  FO_REQUIRE((K & 31) == 0, "%s: K=%d must be a multiple of 32", fn, K);
  FO_REQUIRE(X && Q && Y, "%s: NULL X, Q or Y", fn);
  FO_REQUIRE(scale, "%s: NULL scale (the E8M0 block bytes of fo_quant_w6)", fn);
  FO_REQUIRE(ldx >= K && (ldx & 3) == 0 && ((unsigned long long)X & 15) == 0,
             "%s: X needs ldx=%d >= K=%d, ldx %% 4 == 0 and 16-byte alignment", fn, ldx, K);
  FO_REQUIRE(ldy >= N, "%s: ldy=%d < N=%d", fn, ldy, N);
  units = (N + 15) / 16;
  FO_REQUIRE(!swiglu || (ntiles & 1) == 0, "%s: swiglu with an odd ntiles=%d (gate/up tiles come in pairs)", fn, ntiles);
  // ntiles is the extent of Q and scale (the descriptors' range): (gate, up) pairs for SwiGLU
  FO_REQUIRE(ntiles == (swiglu ? 2 : 1) * units, "%s: ntiles=%d packed tiles for N=%d%s", fn, ntiles, N,
             swiglu ? " SwiGLU columns" : " columns");
  FO_REQUIRE(!rstats || rgroups > 0, "%s: rstats without rgroups", fn);
  FO_REQUIRE(!sout || (!swiglu && (!yg || gnext)), "%s: sout needs a non-SwiGLU launch, yg needs gnext", fn);
  FO_REQUIRE(sout || !yg, "%s: yg comes with sout", fn);
  FO_REQUIRE(!(swiglu && residual), "%s: swiglu with residual unsupported", fn);
  const int KK = (K + 127) / 128;
  FO_REQUIRE((long long)(ntiles + 4) * KK * W6_STEP < (1ll << 31), "%s: ntiles=%d x K=%d codes exceed 2 GiB", fn, ntiles,
             K);
  a = W8Args{X,        Q,    reinterpret_cast<const float*>(scale), Y,  ldx,    ldy,     M, K, N, ntiles, KK,
             residual, sout, gnext,                                 yg, rstats, rgroups, eps};
  return 0;
}

}  // namespace

extern "C" {

long long fo_quant_w6_bytes(int N, int K) { return (long long)((N + 15) / 16) * ((K + 127) / 128) * W6_STEP; }
long long fo_quant_w6_scale_bytes(int N, int K) { return (long long)((N + 15) / 16) * ((K + 127) / 128) * 64; }

int fo_quant_w6(const void* W, int src_bf16, int N, int K, int ldw, void* q, void* scale, void* wdq, int tile_base,
                int tile_stride, hipStream_t stream) {
  FO_REQUIRE(W && q && scale, "fo_quant_w6: NULL W, q or scale");
  FO_REQUIRE(N > 0 && K > 0 && ldw >= K, "fo_quant_w6: bad shape N=%d K=%d ldw=%d", N, K, ldw);
  FO_REQUIRE((K & 31) == 0, "fo_quant_w6: K=%d must be a multiple of 32 (the scale block)", K);
  FO_REQUIRE(tile_base >= 0 && tile_stride >= 1, "fo_quant_w6: bad tile_base=%d tile_stride=%d", tile_base,
             tile_stride);
  const int nt = (N + 15) / 16;
  hipLaunchKernelGGL(k_quant_w6, dim3(nt * 16), dim3(256), 0, stream, W, src_bf16, N, K, ldw, (unsigned char*)q,
                     (unsigned char*)scale, (bf16_t*)wdq, (K + 127) / 128, tile_base, tile_stride);
  return fo::check_launch("fo_quant_w6");
}

int fo_gemm_w6_counts(long long* out, int n) {
  for (int i = 0; out && i < n && i < 4; ++i) out[i] = g_w6_launches[i].load(std::memory_order_relaxed);
  return 4;
}
int fo_gemm_w6_counts_reset(void) {
  for (int i = 0; i < 4; ++i) g_w6_launches[i].store(0, std::memory_order_relaxed);
  g_w6_rows_calls.store(0, std::memory_order_relaxed);
  return 0;
}
long long fo_gemm_w6_rows_count(void) { return g_w6_rows_calls.load(std::memory_order_relaxed); }

int fo_gemm_w6(const float* X, int ldx, int M, int K, const void* Q, const void* scale, int ntiles, int N, int swiglu,
               float* Y, int ldy, int residual, float* ws, long long ws_floats, int* counters, const float* rstats,
               int rgroups, float eps, float* sout, const float* gnext, float* yg, int* sgroups, hipStream_t stream) {
  // every check before the first HIP call
  W8Args a;
  int units;
  if (const int rc = w6_args("fo_gemm_w6", 1, 16, W6_SERVES_16, X, ldx, M, K, Q, scale, ntiles, N, swiglu, Y, ldy,
                             residual, rstats, rgroups, eps, sout, gnext, yg, a, units))
    return rc;
  const int KK = a.KK;
  if (sgroups) *sgroups = units;
  if (swiglu && K == 3584) {
    const int G = units < w6_cus() ? units : w6_cus();
    // 14 waves x 2 code steps; FO_W6_XS=7 runs 7 x 4 (A/B only)
    static const bool w7 = [] { const char* e = getenv("FO_W6_XS"); return e && atoi(e) == 7; }();
    if (w7) hipLaunchKernelGGL((k_w6_xs<7, 4>), dim3(G), dim3(448), 0, stream, a, units);
    else hipLaunchKernelGGL((k_w6_xs<14, 2>), dim3(G), dim3(896), 0, stream, a, units);
    g_w6_launches[1].fetch_add(1, std::memory_order_relaxed);
    return fo::check_launch("fo_gemm_w6 (xs)");
  }
  // long-K plain projections (the Qwen2 down: 224 tiles x 148 code steps): 4 tiles per workgroup, K split over the
  // workgroups until the grid is about one workgroup per CU, merged in the launch (needs the caller's workspace and
  // zeroed tickets; without them the one-tile form below serves)
  if (!swiglu && KK >= 64 && units >= 16 && ws && counters) {
    constexpr int NT = 4, NW = 8;
    const int groups = (units + NT - 1) / NT;
    int S = w6_cus() / groups;
    S = S < 1 ? 1 : (S > 8 ? 8 : S);
    if (S == 1 || ((long long)S * 16 * groups * NT * 16 <= ws_floats && groups <= (1 << 20))) {
      hipLaunchKernelGGL((k_w6_sk<NW, NT>), dim3(groups, S), dim3(NW * 64), 0, stream, a, S, ws, counters);
      g_w6_launches[2].fetch_add(1, std::memory_order_relaxed);
      return fo::check_launch("fo_gemm_w6 (split K)");
    }
  }
  const bool wide = KK >= 16;
  if (swiglu) {
    if (wide) hipLaunchKernelGGL((k_w6<16, true>), dim3(units), dim3(1024), 0, stream, a);
    else hipLaunchKernelGGL((k_w6<4, true>), dim3(units), dim3(256), 0, stream, a);
  } else {
    if (wide) hipLaunchKernelGGL((k_w6<16, false>), dim3(units), dim3(1024), 0, stream, a);
    else hipLaunchKernelGGL((k_w6<4, false>), dim3(units), dim3(256), 0, stream, a);
  }
  g_w6_launches[0].fetch_add(1, std::memory_order_relaxed);
  return fo::check_launch("fo_gemm_w6");
}

int fo_gemm_w6_head(const float* X, int ldx, int M, int K, const void* Q, const void* scale, int ntiles, int N,
                    float* Y, int ldy, hipStream_t stream) {
  // every check before the first HIP call
  W8Args a;
  int tiles;
  if (const int rc = w6_args("fo_gemm_w6_head", 1, 16, W6_SERVES_16, X, ldx, M, K, Q, scale, ntiles, N, 0, Y, ldy, 0,
                             nullptr, 0, 0.f, nullptr, nullptr, nullptr, a, tiles))
    return rc;
  FO_REQUIRE(K == 3584, "fo_gemm_w6_head: K=%d, the X-stationary plain form is compiled for K = 3584 (fo_gemm_w6 serves "
             "any other K)", K);
  // units of two adjacent plain tiles dealt evenly to at most one workgroup per CU; the SwiGLU form's wave shape
  const int units = (ntiles + 1) / 2;
  const int G = units < w6_cus() ? units : w6_cus();
  hipLaunchKernelGGL((k_w6_xs<14, 2, false>), dim3(G), dim3(896), 0, stream, a, units);
  g_w6_launches[3].fetch_add(1, std::memory_order_relaxed);
  return fo::check_launch("fo_gemm_w6_head");
}

int fo_gemm_w6_rows(const float* X, int ldx, int M, int K, const void* Q, const void* scale, int ntiles, int N,
                    int swiglu, float* Y, int ldy, int residual, float* ws, long long ws_floats, int* counters,
                    const float* rstats, int rgroups, float eps, float* sout, const float* gnext, float* yg,
                    int* sgroups, hipStream_t stream) {
  // every check before the first HIP call
  W8Args a;
  int units;
  if (const int rc = w6_args("fo_gemm_w6_rows", 17, 64,
                             "this MXFP6 stream serves 17 <= M <= 64 (fo_gemm_w6 serves M <= 16, more than 64 rows run "
                             "the bf16 image)",
                             X, ldx, M, K, Q, scale, ntiles, N, swiglu, Y, ldy, residual, rstats, rgroups, eps, sout,
                             gnext, yg, a, units))
    return rc;
  const int KK = a.KK;
  // NW waves x KPW code steps of X per K slice (hi in VGPRs, lo in LDS): fo_gemm_w4_rows's shapes at 3 and 4 row
  // blocks (7 x 1 for SwiGLU, 8 x 1 / 6 x 1 for plain).  At 2 row blocks its 7 x 2 does not fit here: the two-deep code
  // buffer is 2 x 2 x KPW x 7 dwords a lane against MXFP4's x 5, and both 7 x 2 instantiations spilled (256 VGPRs, 8 and
  // 16 bytes of scratch a lane), so 2 row blocks run 7 x 1 (DESIGN 5.10 has every instantiation's figures).  S slices
  // of `per` code steps, units of two packed tiles, about one workgroup per CU.  S > 1: the slabs are merged by a
  // second launch (k_w8_rows_merge), one small workgroup per (tile, row block)
  const int RB = (M + 15) / 16;
  const int NW = RB == 3 ? (swiglu ? 7 : 8) : (RB == 4 && !swiglu ? 6 : 7), KPW = 1;
  const int S = (KK + NW * KPW - 1) / (NW * KPW), per = (KK + S - 1) / S;
  if (S > 1) {
    const long long need = (long long)S * RB * 16 * ntiles * 16;
    FO_REQUIRE(ws && need <= ws_floats,
               "fo_gemm_w6_rows: K=%d splits over %d workgroups: split-K workspace too small (%lld floats needed, "
               "%lld given)", K, S, need, ws ? ws_floats : 0ll);
  }
  const int pairs = (ntiles + 1) / 2;
  const int per_split = w6_cus() / S < 1 ? 1 : w6_cus() / S;
  const int G = pairs < per_split ? pairs : per_split;
  (void)counters;
  if (sgroups) *sgroups = units;
  const dim3 grid(G, S), block(NW * 64);
#define FO_W6_ROWS(NW_, KPW_, RB_, SW_) \
  hipLaunchKernelGGL((k_w6_rows<NW_, KPW_, RB_, SW_>), grid, block, 0, stream, a, S, per, ws)
  if (RB == 2) {
    if (swiglu) FO_W6_ROWS(7, 1, 2, true);
    else FO_W6_ROWS(7, 1, 2, false);
  } else if (RB == 3) {
    if (swiglu) FO_W6_ROWS(7, 1, 3, true);
    else FO_W6_ROWS(8, 1, 3, false);
  } else {
    if (swiglu) FO_W6_ROWS(7, 1, 4, true);
    else FO_W6_ROWS(6, 1, 4, false);
  }
#undef FO_W6_ROWS
  if (S > 1) {
    const int rc = fo::check_launch("fo_gemm_w6_rows");
    if (rc) return rc;
    launch_merge<false>(a, swiglu, units, RB, S, ws, stream);
  }
  g_w6_rows_calls.fetch_add(1, std::memory_order_relaxed);
  return fo::check_launch("fo_gemm_w6_rows");
}

}  // extern "C"
