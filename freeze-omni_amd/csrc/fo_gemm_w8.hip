// Weight-only FP8 (OCP e4m3fn) GEMMs for the Qwen2 MLP, and their quantiser.
//
//   W'[n, k] = q[n, k] * 2^e[n]      q an e4m3fn code, e[n] one integer per output row (stored as the fp32 2^e[n])
//   Y[M, N]  = epilogue( X[M, K] (fp32, split into bf16 hi + lo) . W'^T )
//
// An e4m3 value has at most 4 significant bits, so q * 2^e is exactly a bf16 value: W' has an exact bf16 image, which
// the engine keeps packed for the bf16 kernels.  The kernels here stream the codes -- half the bytes of that image --
// decode them to bf16 in registers (exact) and run the same bf16 MFMAs; the column scale multiplies the fp32 sum once
// per output element, before anything else in the epilogue, so both paths compute X . W'^T to the accumulation-order
// difference that already exists between the bf16 kernels.  Results are deterministic in every form.
//
// Code layout (include/fo_hip.h): [tile][K64][64 lanes][16 codes], a lane's 16 bytes being its 8-element MFMA
// B-fragments of two consecutive 32-column k-steps, K padded to a multiple of 64 with zero codes.  One entry per row
// band, each kernel's design above the kernel:
//  * fo_gemm_w8, <= 16 rows: k_w8 (general), k_w8_xs (the SwiGLU pair at K = 3584) or k_w8_sk (long-K plain);
//  * fo_gemm_w8_head, <= 16 rows: k_w8_xs's plain form at K = 3584 (the Qwen2 lm_head);
//  * fo_gemm_w8_qkv_rope, <= 16 rows: k_w8_qkv, k_w8's pair form with the fused q|k|v epilogue (bias, RoPE, paged-KV
//    append: fo_gemm_wq.h) over the rope-paired tile order of PackedLinear(rope_hd=...);
//  * fo_gemm_w8_rows, 17..64 rows: k_w8_rows, then k_w8_rows_merge where K is split;
//  * fo_gemm_w8_rows128, 65..128 rows: k_w8_rows128, then k_w8_rows_merge.
#include <stdlib.h>

#include "fo_gemm_wq.h"

namespace {

// 8 e4m3fn codes (two dwords) -> 8 bf16: v_cvt_pk_f32_fp8 per code pair, then the upper halves of the two floats in
// one v_perm (an e4m3 value has 4 significant bits: the truncation is exact)
__device__ __forceinline__ bf16x8 dec8(unsigned a, unsigned b) {
  const f32x2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a, false), f1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a, true);
  const f32x2 f2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b, false), f3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b, true);
  u32x4 r;
  r[0] = __builtin_amdgcn_perm(__float_as_uint(f0[1]), __float_as_uint(f0[0]), 0x07060302u);
  r[1] = __builtin_amdgcn_perm(__float_as_uint(f1[1]), __float_as_uint(f1[0]), 0x07060302u);
  r[2] = __builtin_amdgcn_perm(__float_as_uint(f2[1]), __float_as_uint(f2[0]), 0x07060302u);
  r[3] = __builtin_amdgcn_perm(__float_as_uint(f3[1]), __float_as_uint(f3[0]), 0x07060302u);
  return __builtin_bit_cast(bf16x8, r);
}

// acc[t] = X[rows 0..16, code steps [kb, ke)] . (packed tile tile0 + t)^T for t < NT: U code steps in flight, each X
// fragment loaded and split once for the NT tiles.  The codes' descriptor covers exactly the codes (ntiles * KK KiB): a
// tile at or past ntiles is out of its range and loads zero codes.
template <int NT, int U>
__device__ __forceinline__ void w8_accumulate(const W8Args& a, __amdgpu_buffer_rsrc_t srd, const float* xp, int voff,
                                              int tile0, int kb, int ke, f32x4 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = kb; k0 < ke; k0 += U) {
    u32x4 q[U][NT];
    float4 x[U][4];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int kk = k0 + i;
      if (kk < ke) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
          q[i][t] = __builtin_bit_cast(
              u32x4, __builtin_amdgcn_raw_buffer_load_b128(srd, voff, ((tile0 + t) * a.KK + kk) * 1024, 2));
        const float* p = xp + (size_t)kk * 64;
        x[i][0] = reinterpret_cast<const float4*>(p)[0];
        x[i][1] = reinterpret_cast<const float4*>(p)[1];
        if (kk * 64 + 32 < a.K) {   // (K % 64 == 32: the last step's second half is zero codes and no X)
          x[i][2] = reinterpret_cast<const float4*>(p + 32)[0];
          x[i][3] = reinterpret_cast<const float4*>(p + 32)[1];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int kk = k0 + i;
      if (kk < ke) {
        bf16x8 hi, lo;
        split8(x[i][0], x[i][1], hi, lo);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const bf16x8 w = dec8(q[i][t][0], q[i][t][1]);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, w, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, w, acc[t], 0, 0, 0);
        }
        if (kk * 64 + 32 < a.K) {
          split8(x[i][2], x[i][3], hi, lo);
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const bf16x8 w = dec8(q[i][t][2], q[i][t][3]);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, w, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, w, acc[t], 0, 0, 0);
          }
        }
      }
    }
  }
}

// ---- general form: workgroup u = output tile u (SW: the (gate, up) pair 2u, 2u + 1); wave w takes the code steps
// [KK w / NW, KK (w + 1) / NW), U of them (per tile) in flight
template <int NW, bool SW>
__global__ __launch_bounds__(NW * 64) void k_w8(W8Args a) {
  constexpr int T = SW ? 2 : 1, U = SW ? 2 : 4;   // (4 pair steps spill at 16 waves' 128 VGPRs)
  __shared__ float part[NW][T][16][17];
  __shared__ float rstd_s[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = blockIdx.x;
  const __amdgpu_buffer_rsrc_t srd = rsrc_of(a.Q, a.ntiles * a.KK * 1024);
  const int kb = (int)((long)a.KK * wave / NW), ke = (int)((long)a.KK * (wave + 1) / NW);
  const int row = min(lane & 15, a.M - 1);
  const float* xp = a.X + (size_t)row * a.ldx + 8 * (lane >> 4);
  const int voff = lane * 16;
  if (a.rstats) w8_rstd<NW>(a, rstd_s, wave, lane);
  f32x4 acc[T];
  w8_accumulate<T, U>(a, srd, xp, voff, T * u, kb, ke, acc);
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
    w8_epilogue<SW>(a, u, gridDim.x, rr, c, x1, x2, rstd_s);
  }
}

// ---- the fused q|k|v projection (fo_gemm_w8_qkv_rope): k_w8's pair form with the RoPE + paged-KV epilogue in place
// of SwiGLU.  Workgroup P = rope tile pair P (packed tiles 2P, 2P + 1: columns (i, i + hd/2) of one head); the waves
// split the code steps as in k_w8 and the cross-wave sum runs in wave order.  No workspace, no tickets.
template <int NW>
__global__ __launch_bounds__(NW * 64) void k_w8_qkv(W8Args a, QkvRopeArgs r) {
  constexpr int U = 2;
  __shared__ float part[NW][2][16][17];
  __shared__ float rstd_s[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int P = blockIdx.x;
  const __amdgpu_buffer_rsrc_t srd = rsrc_of(a.Q, a.ntiles * a.KK * 1024);
  const int kb = (int)((long)a.KK * wave / NW), ke = (int)((long)a.KK * (wave + 1) / NW);
  const int row = min(lane & 15, a.M - 1);
  const float* xp = a.X + (size_t)row * a.ldx + 8 * (lane >> 4);
  const int voff = lane * 16;
  if (a.rstats) w8_rstd<NW>(a, rstd_s, wave, lane);
  f32x4 acc[2];
  w8_accumulate<2, U>(a, srd, xp, voff, 2 * P, kb, ke, acc);
  w8_store_tile(part[wave][0], acc[0], lane);
  w8_store_tile(part[wave][1], acc[1], lane);
  __syncthreads();
  const int e = threadIdx.x;
  if (e < 256) {
    const int rr = e >> 4, c = e & 15;
    float x1 = 0.f, x2 = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      x1 += part[w][0][rr][c];
      x2 += part[w][1][rr][c];
    }
    wq_rope_epilogue<true>(a, r, P, rr, c, x1, x2, rstd_s);
  }
}

// ---- long-K plain form: workgroup (tg, sp) = tiles NT tg .. + NT over the sp-th of S slices of the code steps, the
// slice split over the waves as in k_w8.  ws: S slabs of [16][groups * NT * 16] partial sums; counters: one zeroed
// ticket per tile group, left zeroed.  The hand-off is fo_common.h's (st_wt / ld_sc1): no fences, no waiting.
template <int NW, int NT>
__global__ __launch_bounds__(NW * 64) void k_w8_sk(W8Args a, int S, float* ws, int* counters) {
  constexpr int U = 2;
  __shared__ float part[NW][NT][16][17];
  __shared__ float red[NT][16][17];
  __shared__ float rstd_s[16];
  __shared__ int last_s;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tg = blockIdx.x, sp = blockIdx.y;
  const __amdgpu_buffer_rsrc_t srd = rsrc_of(a.Q, a.ntiles * a.KK * 1024);
  const int k_lo = (int)((long)a.KK * sp / S), k_n = (int)((long)a.KK * (sp + 1) / S) - k_lo;
  const int kb = k_lo + (int)((long)k_n * wave / NW), ke = k_lo + (int)((long)k_n * (wave + 1) / NW);
  const int row = min(lane & 15, a.M - 1);
  const float* xp = a.X + (size_t)row * a.ldx + 8 * (lane >> 4);
  const int voff = lane * 16;
  if (a.rstats) w8_rstd<NW>(a, rstd_s, wave, lane);
  f32x4 acc[NT];
  w8_accumulate<NT, U>(a, srd, xp, voff, NT * tg, kb, ke, acc);
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
    // the last split to arrive: every split's partial, summed in split order
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
      if (tg * NT + t < units) w8_epilogue<false>(a, tg * NT + t, units, rr, c, red[t][rr][c], 0.f, rstd_s);
  }
}

// ---- X-stationary persistent form, as k_gemm_xs (fo_gemm.hip): the SwiGLU pair, K = NW * KPW * 64 (3584 = 56 code
// steps).  X hi in registers, lo in LDS, units dealt evenly to at most one workgroup per CU, the next unit's codes
// issued before the current one is reduced, a fixed-order cross-wave reduction.
// SW = false (fo_gemm_w8_head): the plain form.  A unit is two adjacent plain tiles 2u, 2u + 1 (the second of an odd
// count's last unit lies past the code descriptor and loads zero codes; it is never stored), each with the plain
// epilogue: the column scale and the store, no residual, no statistics (NW * 64 >= 512: a tile per 256 threads).
template <int NW, int KPW, bool SW = true>
__global__ __launch_bounds__(NW * 64) void k_w8_xs(W8Args a, int units) {
  static_assert(SW || NW >= 8, "k_w8_xs: the plain epilogue takes 512 threads");
  __shared__ bf16x8 xlo[NW][2 * KPW][64];
  __shared__ float part[NW][2][16][17];
  __shared__ float rstd_s[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int KK = NW * KPW;
  const int ub = (int)((long)units * blockIdx.x / gridDim.x);
  const int ue = (int)((long)units * (blockIdx.x + 1) / gridDim.x);
  const __amdgpu_buffer_rsrc_t srd = rsrc_of(a.Q, a.ntiles * a.KK * 1024);   // (exactly the codes)
  const int voff = (wave * KPW * 64 + lane) * 16;
  u32x4 q0[KPW], q1[KPW];
  auto issue = [&](u32x4 (&q)[KPW], int tile) {
#pragma unroll
    for (int j = 0; j < KPW; ++j)
      q[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(srd, voff, (tile * KK + j) * 1024, 2));
  };
  issue(q0, ub < ue ? 2 * ub : a.ntiles);
  issue(q1, ub < ue ? 2 * ub + 1 : a.ntiles);
  // X slice (hi in registers, lo in LDS); rows >= M clamp to the last row (computed, never stored)
  bf16x8 xh[2 * KPW];
  {
    const int row = min(lane & 15, a.M - 1);
    const float* xp = a.X + (size_t)row * a.ldx + 8 * (lane >> 4) + (size_t)wave * KPW * 64;
#pragma unroll
    for (int j = 0; j < 2 * KPW; ++j) {
      bf16x8 lo;
      split8(reinterpret_cast<const float4*>(xp + j * 32)[0], reinterpret_cast<const float4*>(xp + j * 32)[1], xh[j],
             lo);
      xlo[wave][j][lane] = lo;
    }
  }
  if constexpr (SW) {
    if (a.rstats) w8_rstd<NW>(a, rstd_s, wave, lane);
  }
  auto compute = [&](u32x4 (&q)[KPW]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < KPW; ++j) {
      const bf16x8 w0 = dec8(q[j][0], q[j][1]), w1 = dec8(q[j][2], q[j][3]);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[2 * j], w0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xlo[wave][2 * j][lane], w0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[2 * j + 1], w1, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xlo[wave][2 * j + 1][lane], w1, acc, 0, 0, 0);
    }
    return acc;
  };
  for (int u = ub; u < ue; ++u) {
    // the next unit's codes are issued unconditionally; past the last unit they address tile `ntiles`, beyond the
    // descriptor's range, which the hardware drops without touching memory
    const int nxt = u + 1 < ue ? 2 * (u + 1) : a.ntiles;
    const f32x4 c0 = compute(q0);
    issue(q0, nxt);
    const f32x4 c1 = compute(q1);
    issue(q1, nxt + (u + 1 < ue ? 1 : 0));
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
        w8_epilogue<true>(a, u, 0, rr, c, x1, x2, rstd_s);
      }
    } else if (e < 512) {
      const int t = e >> 8, rr = (e >> 4) & 15, c = e & 15;
      float x1 = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) x1 += part[w][t][rr][c];
      if (2 * u + t < a.ntiles) w8_epilogue<false>(a, 2 * u + t, 0, rr, c, x1, 0.f, rstd_s);
    }
  }
}

// ---- 17..64 rows (RB = 2..4 row blocks of 16): X-stationary with K split over workgroups, k_gemm_xsk's design
// (fo_gemm.hip) on the codes.  Workgroup (g, sp): the sp-th of S slices of the code steps for units [ub, ue) of
// column group g; a unit is a packed tile pair (the (gate, up) pair, or two adjacent plain tiles: the second of an
// odd count's last pair lies past the code descriptor and loads zeros).  Wave w owns KPW code steps of the slice:
// their X fragments of all RB row blocks are split once (hi in VGPRs, lo in its LDS region; k-steps at or past K
// hold zeros and read no X), each 16-byte code load is decoded once per unit (dec8) and feeds RB x (hi, lo) MFMAs per
// k-step, the next unit's codes in flight meanwhile.  Per unit the NW partial tiles are summed through LDS in wave
// order (both tiles in one round where the LDS allows).  S == 1: the epilogue follows.  S > 1: the sums are stored as
// split sp's slab of `ws` ([S][RB * 16][ntiles * 16] floats) and k_w8_rows_merge, the next launch, sums the slabs in
// split order and runs the epilogue.
template <int NW, int KPW, int RB, bool SW>
__global__ __launch_bounds__(NW * 64) void k_w8_rows(W8Args a, int S, int per, float* ws) {
  constexpr int ROWS = RB * 16, NTH = NW * 64, NE = ROWS * 16, EPT = (NE + NTH - 1) / NTH;
  constexpr int PT = (NW * RB * 2 * KPW * 1024 + NW * 2 * ROWS * 17 * 4 + 512 <= 160 * 1024) ? 2 : 1;
  __shared__ bf16x8 xlo[NW][RB][2 * KPW][64];
  __shared__ float part[NW][PT][ROWS][17];
  __shared__ float rstd_s[ROWS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int G = gridDim.x, g = blockIdx.x, sp = blockIdx.y;
  const int units = (a.ntiles + 1) >> 1, tiles = (a.N + 15) / 16;   // (tiles: output tiles, the statistics' groups)
  const int ub = (int)((long)units * g / G), ue = (int)((long)units * (g + 1) / G);
  const __amdgpu_buffer_rsrc_t srd = rsrc_of(a.Q, a.ntiles * a.KK * 1024);   // (exactly the codes)
  // this wave's code steps: [k0, k0 + nj) inside the slice [sp * per, (sp + 1) * per) and inside KK (wave-uniform)
  const int k0 = sp * per + wave * KPW;
  const int nj = max(0, min(KPW, min(a.KK, (sp + 1) * per) - k0));
  const int voff = lane * 16;
  u32x4 q[2][2][KPW];
  auto issue = [&](u32x4 (&qq)[2][KPW], int u) {   // u >= ue: past the workgroup's range, no load issued
    if (u < ue) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < KPW; ++j)
          if (j < nj)
            qq[t][j] = __builtin_bit_cast(
                u32x4, __builtin_amdgcn_raw_buffer_load_b128(srd, voff, ((2 * u + t) * a.KK + k0 + j) * 1024, 2));
    }
  };
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < KPW; ++j) q[b][t][j] = u32x4{0u, 0u, 0u, 0u};   // code steps past the slice: zero codes
  issue(q[0], ub);
  issue(q[1], ub + 1);
  bf16x8 zero;
#pragma unroll
  for (int i = 0; i < 8; ++i) zero[i] = (__bf16)0.f;
  bf16x8 xh[RB][2 * KPW];
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const int row = min(r * 16 + (lane & 15), a.M - 1);   // rows >= M: computed, never stored or summed
    const float* xp = a.X + (size_t)row * a.ldx + 8 * (lane >> 4);
#pragma unroll
    for (int j = 0; j < 2 * KPW; ++j) {
      bf16x8 hi = zero, lo = zero;
      const int col = (2 * k0 + j) * 32;   // (K % 64 == 32: the last code step's second k-step is past K)
      if ((j >> 1) < nj && col < a.K)
        split8(reinterpret_cast<const float4*>(xp + col)[0], reinterpret_cast<const float4*>(xp + col)[1], hi, lo);
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
  auto unit = [&](u32x4 (&qq)[2][KPW], int u) {
    float v[2][EPT];
#pragma unroll
    for (int t0 = 0; t0 < 2; t0 += PT) {
      f32x4 acc[PT][RB];
#pragma unroll
      for (int p = 0; p < PT; ++p) {
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[p][r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KPW; ++j)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const bf16x8 w = dec8(qq[t0 + p][j][2 * h], qq[t0 + p][j][2 * h + 1]);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
              acc[p][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[r][2 * j + h], w, acc[p][r], 0, 0, 0);
              acc[p][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xlo[wave][r][2 * j + h][lane], w, acc[p][r], 0, 0, 0);
            }
          }
      }
      if (t0 + PT == 2) issue(qq, u + 2);   // (the unit's codes are decoded: its buffer takes the unit after next)
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
          w8_epilogue<true>(a, u, tiles, rr, c, v[0][i], v[1][i], rstd_s);
        } else {
          w8_epilogue<false>(a, 2 * u, tiles, rr, c, v[0][i], 0.f, rstd_s);
          if (2 * u + 1 < a.ntiles) w8_epilogue<false>(a, 2 * u + 1, tiles, rr, c, v[1][i], 0.f, rstd_s);
        }
      }
    }
  };
  for (int u = ub; u < ue; u += 2) {   // (workgroup-uniform: every wave reaches unit's barriers)
    unit(q[0], u);
    if (u + 1 < ue) unit(q[1], u + 1);
  }
}

// (k_w8_rows_merge, the merge of k_w8_rows's and k_w8_rows128's slabs, is fo_gemm_wq.h's with the column scale.)

// ---- 65..128 rows (fo_gemm_w8_rows128): k_gemm_rows's design (fo_gemm.hip) on the codes.  The 8 waves of a
// workgroup split the row blocks (wave w: rows 16 w .. + 16; a wave past ceil(M / 16) only carries its share of the
// loads) and share each code step's weight fragments through LDS: no cross-wave reduction, every code read from HBM
// once.  Workgroup (sp, gx): the sp-th of S slices of the code steps for the packed tiles [gx tiles_per, + tiles_per).
//  * one LDS-DMA loader ring per workgroup, advanced per 64-column code step, weights and X both D code steps ahead
//    (vmcnt retires in order: a shorter X lead would cap the weights' depth, see launch_rows in fo_gemm.hip): per slot
//    one 1 KiB code fragment per tile -- a lane's 16 bytes are its B fragments of the step's two k-steps, so one
//    dma16 moves what takes the bf16 image two -- and the fp32 rows of every row block for both k-steps (4 KiB per row
//    block, k_gemm_rows's lane map, one load per 8 rows x 32 columns);
//  * per code step: one s_waitcnt on the wave's own DMA (every step padded to the same OPS loads), one barrier, the
//    wave's two X fragments split into bf16 hi / lo, then per tile one 16-byte LDS read, two dec8 and four MFMAs
//    (hi and lo of each k-step), in groups of TG tiles so that no accumulator is read right after it is written,
//    the next group's decode interleaved with the current group's MFMAs;
//  * K % 64 == 32: the last code step's second k-step is zero codes; its X is not loaded and zeros are multiplied;
//  * the fp32 partial tiles go to slice sp's slab of `ws` ([S][16 ceil(M/16)][ntiles * 16]) with plain stores;
//    k_w8_rows_merge, the next launch, sums the slabs in slice order and runs the epilogue.
template <int N>
__device__ __forceinline__ void w8_wait_vm_barrier() {
  // this wave's DMA down to N outstanding and its LDS reads done, then the workgroup barrier, in one opaque statement
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"i"(N) : "memory");
}

template <int NTC, int D>
__global__ __launch_bounds__(512) void k_w8_rows128(W8Args a, int S, int G, int tiles_per, float* ws) {
  constexpr int NWV = 8, P = D + 1;
  constexpr int LPW = (NTC + NWV - 1) / NWV;   // code loads per wave per code step (tile t: wave t % 8)
  constexpr int OPS = LPW + 4;                 // DMA loads per wave per code step
  constexpr int TG = NTC % 8 == 0 ? 8 : (NTC % 7 == 0 ? 7 : (NTC % 6 == 0 ? 6 : 5));
  static_assert(NTC % TG == 0, "k_w8_rows128: tile groups");
  static_assert(P * (NTC + 32) * 1024 + 1024 <= 160 * 1024, "k_w8_rows128: LDS");
  __shared__ u32x4 wr[P][NTC][64];          // code ring: one 1 KiB fragment (two k-steps) per (slot, tile)
  __shared__ float4 xr[P][NWV][2][2][64];   // X ring: [slot][row block][k-step of the code step][row half][lane]
  __shared__ float4 dummy[64];              // the padding loads land here
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int total = S * G, per_x = (total + 7) >> 3;
  const int wgi = (int)(blockIdx.x & 7) * per_x + (int)(blockIdx.x >> 3);   // (XCD-aware, as k_gemm_rows)
  if (wgi >= total) return;
  const int sp = wgi / G, gx = wgi - sp * G;
  const int tb = gx * tiles_per, nt = min(a.ntiles, tb + tiles_per) - tb;   // nt <= NTC (host)
  const int kb = (int)((long)a.KK * sp / S), nk = (int)((long)a.KK * (sp + 1) / S) - kb;
  const bool live = wave * 16 < a.M;
  const char* wbase = reinterpret_cast<const char*>(a.Q);
  // this lane's X row of the wave's row block (rows >= M clamp to M - 1: computed, never stored)
  const float* xrow[2];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    const int row = min(wave * 16 + 8 * hf + (lane & 7), a.M - 1);
    const int c = ((lane >> 3) - hf) & 7;
    xrow[hf] = a.X + (size_t)row * a.ldx + 4 * c;
  }
  // the consumer's two LDS slots (16-B lanes of the two loads' images)
  const int xh0 = (lane & 15) >> 3;
  const int xs0 = (16 * (lane >> 4) + (lane & 7) + 8 * xh0) & 63, xs1 = (xs0 + 8) & 63;
  const unsigned dummy_l = __builtin_amdgcn_readfirstlane(lds_addr(&dummy[0]));
  const void* dummy_g = wbase + (size_t)lane * 16;
  // code step i (relative to kb) into ring slot i % P: the wave's tiles, then its row block's X of both k-steps
  auto issue = [&](int i) {
#pragma unroll
    for (int q = 0; q < LPW; ++q) {
      const int t = q * NWV + wave;
      if (i < nk && t < nt && t < NTC) {
        const void* src = wbase + ((size_t)(tb + t) * a.KK + (kb + i)) * 1024 + (size_t)lane * 16;
        dma16(src, __builtin_amdgcn_readfirstlane(lds_addr(&wr[i % P][t][0])));
      } else {
        dma16(dummy_g, dummy_l);
      }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int col = (kb + i) * 64 + ks * 32;
        if (i < nk && live && col < a.K) {
          dma16(xrow[hf] + col, __builtin_amdgcn_readfirstlane(lds_addr(&xr[i % P][wave][ks][hf][0])));
        } else {
          dma16(dummy_g, dummy_l);
        }
      }
  };
  f32x4 acc[NTC];
#pragma unroll
  for (int t = 0; t < NTC; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < D; ++j) issue(j);
  for (int i = 0; i < nk; ++i) {
    // this wave's loads of code step i have landed; after the barrier every wave's have, and every wave is done
    // reading step i - 1's slot, which the loads below overwrite
    w8_wait_vm_barrier<(D - 1) * OPS>();
    issue(i + D);
    if (live) {   // (wave-uniform; tiles past nt are computed on whatever the slot holds and never stored)
      const int s = i % P;
      const bool two = (kb + i) * 64 + 32 < a.K;
      bf16x8 xh[2], xl[2];
      split8(xr[s][wave][0][xh0][xs0], xr[s][wave][0][xh0][xs1], xh[0], xl[0]);
      split8(xr[s][wave][1][xh0][xs0], xr[s][wave][1][xh0][xs1], xh[1], xl[1]);
      if (!two) {   // (a select, not a branch: the zero codes of a K % 64 == 32 tail meet zeros, never the stale slot)
#pragma unroll
        for (int e = 0; e < 8; ++e) xh[1][e] = xl[1][e] = (__bf16)0.f;
      }
      // Phase p = 2 g + h: k-step h of tile group g.  Every wave decodes the same codes, so the loop is bound by the
      // VALU decode beside the MFMAs unless the two overlap: phase p + 1's fragments are decoded (8 VALU per tile)
      // between phase p's 2 TG MFMAs, one MFMA : 4 VALU, fixed by the scheduling barriers below (one basic block).
      constexpr int NPH = 2 * (NTC / TG);
      u32x4 q[TG];
      bf16x8 w[2][TG];
#pragma unroll
      for (int t = 0; t < TG; ++t) q[t] = wr[s][t][lane];
#pragma unroll
      for (int t = 0; t < TG; ++t) w[0][t] = dec8(q[t][0], q[t][1]);
#pragma unroll
      for (int p = 0; p < NPH; ++p) {
        const int t0 = (p >> 1) * TG, h = p & 1;
        if (p + 1 < NPH) {
          if (h == 1) {
#pragma unroll
            for (int t = 0; t < TG; ++t) q[t] = wr[s][t0 + TG + t][lane];
#pragma unroll
            for (int t = 0; t < TG; ++t) w[0][t] = dec8(q[t][0], q[t][1]);
          } else {
#pragma unroll
            for (int t = 0; t < TG; ++t) w[1][t] = dec8(q[t][2], q[t][3]);
          }
        }
#pragma unroll
        for (int t = 0; t < TG; ++t)
          acc[t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[h], w[h][t], acc[t0 + t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < TG; ++t)
          acc[t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl[h], w[h][t], acc[t0 + t], 0, 0, 0);
        if (p + 1 < NPH) {
#pragma unroll
          for (int j = 0; j < 2 * TG; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA of this phase
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);   // four VALU of the next phase's decode
          }
        }
      }
    }
  }
  wait_vm<0>();   // (the padding loads past the last code step) nothing of this workgroup's DMA outlives it
  if (!live) return;
  const int Ncols = a.ntiles * 16, rows = ((a.M + 15) >> 4) * 16;
  float* slab = ws + (size_t)sp * rows * Ncols;
#pragma unroll
  for (int t = 0; t < NTC; ++t)
    if (t < nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = wave * 16 + 4 * (lane >> 4) + e;
        if (row < a.M) slab[(size_t)row * Ncols + (tb + t) * 16 + (lane & 15)] = acc[t][e];
      }
}

// ---- quantiser.  One workgroup per source row n: the row's amax, e[n] from its exponent and mantissa (the smallest
// integer with amax * 2^-e <= 448 = 1.75 * 2^8), then 8 consecutive columns per thread: W * 2^-e (exact) rounded to
// nearest-even e4m3fn by v_cvt_pk_fp8_f32, the 8 codes to their fragment position and the 8 dequantised bf16 values
// to wdq.  Rows N .. 16 ceil(N / 16) of the last tile get zero codes and scale 1.
__global__ __launch_bounds__(256) void k_quant_w8(const void* W, int src_bf16, int N, int K, int ldw, unsigned char* q,
                                                  float* scale, bf16_t* wdq, int KK, int tile_base, int tile_stride) {
  __shared__ float red[4];
  const int n = blockIdx.x;
  const int lane = threadIdx.x & 63;
  auto at = [&](int k) {
    return src_bf16 ? bf2f(reinterpret_cast<const bf16_t*>(W)[(size_t)n * ldw + k])
                    : reinterpret_cast<const float*>(W)[(size_t)n * ldw + k];
  };
  float amax = 0.f;
  if (n < N)
    for (int k = threadIdx.x; k < K; k += 256) amax = fmaxf(amax, fabsf(at(k)));
  amax = wave_max(amax);
  if (lane == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const int e = e4m3_row_exp(amax);
  const float s = pow2f(e), inv = pow2f(-e);
  const size_t dt = (size_t)tile_base + (size_t)(n >> 4) * tile_stride;
  if (threadIdx.x == 0) scale[dt * 16 + (n & 15)] = s;
  for (int g = threadIdx.x; g < KK * 8; g += 256) {   // group g: columns 8 g .. + 8
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 8 * g + j;
      v[j] = (n < N && k < K) ? at(k) * inv : 0.f;
    }
    int c0 = 0, c1 = 0;
    c0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], c0, false);
    c0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], c0, true);
    c1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], c1, false);
    c1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], c1, true);
    // column k of row n: code step k / 64, lane 16 (k % 32 / 8) + n % 16, byte 8 (k % 64 / 32) + k % 8
    const int kk = g >> 3, half = (g >> 2) & 1, l = ((g & 3) << 4) + (n & 15);
    *reinterpret_cast<uint2*>(q + ((dt * KK + kk) * 64 + l) * 16 + 8 * half) = make_uint2((unsigned)c0, (unsigned)c1);
    if (wdq && n < N) {
      const bf16x8 d = dec8((unsigned)c0, (unsigned)c1);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (8 * g + j < K) wdq[(size_t)n * K + 8 * g + j] = f2bf((float)d[j] * s);
    }
  }
}

int g_cus = 0;
int w8_cus() {
  if (!g_cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    g_cus = n;
  }
  return g_cus;
}

// What the three GEMM entries share: the checks of everything but the workspace (all before the entry's first HIP
// call), then W8Args (with KK) and the output tile count.  `fn` is the entry's name, [m_lo, m_hi] its row band and
// `serves` what its refusal says of the band.
int w8_args(const char* fn, int m_lo, int m_hi, const char* serves, const float* X, int ldx, int M, int K, const void* Q,
            const float* scale, int ntiles, int N, int swiglu, float* Y, int ldy, int residual, const float* rstats,
            int rgroups, float eps, float* sout, const float* gnext, float* yg, W8Args& a, int& units) {
  FO_REQUIRE(M > 0 && N > 0 && K > 0, "%s: bad shape M=%d N=%d K=%d", fn, M, N, K);
  FO_REQUIRE(M >= m_lo && M <= m_hi, "%s: M=%d rows, %s", fn, M, serves);
  FO_REQUIRE((K & 31) == 0, "%s: K=%d must be a multiple of 32", fn, K);
  FO_REQUIRE(X && Q && Y, "%s: NULL X, Q or Y", fn);
  FO_REQUIRE(scale, "%s: NULL scale (the per-column 2^e of fo_quant_w8)", fn);
  FO_REQUIRE(ldx >= K && (ldx & 3) == 0 && ((unsigned long long)X & 15) == 0,
             "%s: X needs ldx=%d >= K=%d, ldx %% 4 == 0 and 16-byte alignment", fn, ldx, K);
  FO_REQUIRE(ldy >= N, "%s: ldy=%d < N=%d", fn, ldy, N);
  units = (N + 15) / 16;
  // ntiles is the extent of Q and scale (the code descriptor's range): (gate, up) pairs for SwiGLU
  FO_REQUIRE(ntiles == (swiglu ? 2 : 1) * units, "%s: ntiles=%d packed tiles for N=%d%s", fn, ntiles, N,
             swiglu ? " SwiGLU columns" : " columns");
  FO_REQUIRE(!rstats || rgroups > 0, "%s: rstats without rgroups", fn);
  FO_REQUIRE(!sout || (!swiglu && (!yg || gnext)), "%s: sout needs a non-SwiGLU launch, yg needs gnext", fn);
  FO_REQUIRE(sout || !yg, "%s: yg comes with sout", fn);
  FO_REQUIRE(!(swiglu && residual), "%s: swiglu with residual unsupported", fn);
  const int KK = (K + 63) / 64;
  FO_REQUIRE((long long)(ntiles + 4) * KK * 1024 < (1ll << 31), "%s: ntiles=%d x K=%d codes exceed 2 GiB", fn, ntiles, K);
  a = W8Args{X, Q, scale, Y, ldx, ldy, M, K, N, ntiles, KK, residual, sout, gnext, yg, rstats, rgroups, eps};
  return 0;
}

}  // namespace

extern "C" {

long long fo_quant_w8_bytes(int N, int K) { return (long long)((N + 15) / 16) * ((K + 63) / 64) * 1024; }

int fo_quant_w8(const void* W, int src_bf16, int N, int K, int ldw, void* q, float* scale, void* wdq, int tile_base,
                int tile_stride, hipStream_t stream) {
  FO_REQUIRE(W && q && scale, "fo_quant_w8: NULL W, q or scale");
  FO_REQUIRE(N > 0 && K > 0 && ldw >= K, "fo_quant_w8: bad shape N=%d K=%d ldw=%d", N, K, ldw);
  FO_REQUIRE(tile_base >= 0 && tile_stride >= 1, "fo_quant_w8: bad tile_base=%d tile_stride=%d", tile_base,
             tile_stride);
  const int nt = (N + 15) / 16;
  hipLaunchKernelGGL(k_quant_w8, dim3(nt * 16), dim3(256), 0, stream, W, src_bf16, N, K, ldw, (unsigned char*)q, scale,
                     (bf16_t*)wdq, (K + 63) / 64, tile_base, tile_stride);
  return fo::check_launch("fo_quant_w8");
}

int fo_gemm_w8(const float* X, int ldx, int M, int K, const void* Q, const float* scale, int ntiles, int N, int swiglu,
               float* Y, int ldy, int residual, float* ws, long long ws_floats, int* counters, const float* rstats,
               int rgroups, float eps, float* sout, const float* gnext, float* yg, int* sgroups, hipStream_t stream) {
  FO_REQUIRE(!swiglu || (ntiles & 1) == 0, "fo_gemm_w8: swiglu with an odd ntiles=%d (gate/up tiles come in pairs)",
             ntiles);
  W8Args a;
  int units;
  if (const int rc = w8_args("fo_gemm_w8", 1, 16, "the FP8 stream serves M <= 16 (more rows run the bf16 image)", X, ldx,
                             M, K, Q, scale, ntiles, N, swiglu, Y, ldy, residual, rstats, rgroups, eps, sout, gnext, yg,
                             a, units))
    return rc;
  const int KK = a.KK;
  if (sgroups) *sgroups = units;
  if (swiglu && K == 3584) {
    const int G = units < w8_cus() ? units : w8_cus();
    // 14 waves x 4 code steps (25.4 / 28.5 us at 8 / 16 rows against 27.0 / 29.4 for 8 x 7, which FO_W8_XS=8 runs:
    // A/B only)
    static const bool w8 = [] { const char* e = getenv("FO_W8_XS"); return e && atoi(e) == 8; }();
    if (w8) hipLaunchKernelGGL((k_w8_xs<8, 7>), dim3(G), dim3(512), 0, stream, a, units);
    else hipLaunchKernelGGL((k_w8_xs<14, 4>), dim3(G), dim3(896), 0, stream, a, units);
    fo::count_launch(FO_L_GEMM_W8_XS);
    return fo::check_launch("fo_gemm_w8 (xs)");
  }
  // long-K plain projections (the Qwen2 down: 224 tiles x 296 code steps): 4 tiles per workgroup, K split over the
  // workgroups until the grid is about one workgroup per CU, merged in the launch (needs the caller's workspace and
  // zeroed tickets; without them the one-tile form below serves)
  if (!swiglu && KK >= 128 && units >= 16 && ws && counters) {
    constexpr int NT = 4, NW = 8;
    const int groups = (units + NT - 1) / NT;
    int S = w8_cus() / groups;
    S = S < 1 ? 1 : (S > 8 ? 8 : S);
    if (S == 1 || ((long long)S * 16 * groups * NT * 16 <= ws_floats && groups <= (1 << 20))) {
      hipLaunchKernelGGL((k_w8_sk<NW, NT>), dim3(groups, S), dim3(NW * 64), 0, stream, a, S, ws, counters);
      fo::count_launch(FO_L_GEMM_W8);
      return fo::check_launch("fo_gemm_w8 (split K)");
    }
  }
  const bool wide = KK >= 32;
  if (swiglu) {
    if (wide) hipLaunchKernelGGL((k_w8<16, true>), dim3(units), dim3(1024), 0, stream, a);
    else hipLaunchKernelGGL((k_w8<4, true>), dim3(units), dim3(256), 0, stream, a);
  } else {
    if (wide) hipLaunchKernelGGL((k_w8<16, false>), dim3(units), dim3(1024), 0, stream, a);
    else hipLaunchKernelGGL((k_w8<4, false>), dim3(units), dim3(256), 0, stream, a);
  }
  fo::count_launch(FO_L_GEMM_W8);
  return fo::check_launch("fo_gemm_w8");
}

int fo_gemm_w8_head(const float* X, int ldx, int M, int K, const void* Q, const float* scale, int ntiles, int N,
                    float* Y, int ldy, hipStream_t stream) {
  // every check before the first HIP call
  W8Args a;
  int tiles;
  if (const int rc = w8_args("fo_gemm_w8_head", 1, 16, "the FP8 head stream serves M <= 16 (more rows run the bf16 image)",
                             X, ldx, M, K, Q, scale, ntiles, N, 0, Y, ldy, 0, nullptr, 0, 0.f, nullptr, nullptr, nullptr,
                             a, tiles))
    return rc;
  FO_REQUIRE(K == 3584, "fo_gemm_w8_head: K=%d, the X-stationary plain form is compiled for K = 3584 (fo_gemm_w8 serves "
             "any other K)", K);
  // units of two adjacent plain tiles dealt evenly to at most one workgroup per CU; the SwiGLU form's wave shape
  // (14 waves x 4 code steps)
  const int units = (ntiles + 1) / 2;
  const int G = units < w8_cus() ? units : w8_cus();
  hipLaunchKernelGGL((k_w8_xs<14, 4, false>), dim3(G), dim3(896), 0, stream, a, units);
  fo::count_head(0);
  return fo::check_launch("fo_gemm_w8_head");
}

int fo_gemm_w8_qkv_rope(const float* X, int ldx, int M, int K, const void* Q, const float* scale, int ntiles, int N,
                        const float* bias, const float* rstats, int rgroups, float eps, const int* pos, const int* slot,
                        const float* cos_t, const float* sin_t, float* q_out, void* kc, void* vc, int H, int KVH, int hd,
                        int PS, int kv_bytes, hipStream_t stream) {
  // every check before the first HIP call (q_out stands where w8_args expects an output: N floats per row)
  W8Args a;
  QkvRopeArgs r;
  int tiles;
  if (const int rc = w8_args("fo_gemm_w8_qkv_rope", 1, 16,
                             "the FP8 q|k|v stream serves M <= 16 (more rows run the bf16 image)", X, ldx, M, K, Q,
                             scale, ntiles, N, 0, q_out, N, 0, rstats, rgroups, eps, nullptr, nullptr, nullptr, a, tiles))
    return rc;
  if (const int rc = qkv_rope_args("fo_gemm_w8_qkv_rope", N, bias, pos, slot, cos_t, sin_t, q_out, kc, vc, H, KVH, hd,
                                   PS, kv_bytes, r))
    return rc;
  // one workgroup per rope tile pair (Qwen2-7B: 144); 16 waves where each still gets two code steps
  const int pairs = ntiles / 2;
  if (a.KK >= 32) hipLaunchKernelGGL((k_w8_qkv<16>), dim3(pairs), dim3(1024), 0, stream, a, r);
  else hipLaunchKernelGGL((k_w8_qkv<4>), dim3(pairs), dim3(256), 0, stream, a, r);
  fo::count_qkv_quant(0);
  return fo::check_launch("fo_gemm_w8_qkv_rope");
}

int fo_gemm_w8_rows(const float* X, int ldx, int M, int K, const void* Q, const float* scale, int ntiles, int N,
                    int swiglu, float* Y, int ldy, int residual, float* ws, long long ws_floats, int* counters,
                    const float* rstats, int rgroups, float eps, float* sout, const float* gnext, float* yg,
                    int* sgroups, hipStream_t stream) {
  W8Args a;
  int units;
  if (const int rc = w8_args("fo_gemm_w8_rows", 17, 64,
                             "this FP8 stream serves 17 <= M <= 64 (fo_gemm_w8 serves M <= 16, more than 64 rows run the "
                             "bf16 image)",
                             X, ldx, M, K, Q, scale, ntiles, N, swiglu, Y, ldy, residual, rstats, rgroups, eps, sout,
                             gnext, yg, a, units))
    return rc;
  const int KK = a.KK;
  // NW waves x KPW code steps of X per K slice (hi in VGPRs, lo in LDS): 7 x 4 at 2 row blocks, 7 x 2 at 3 and 6 x 2
  // at 4, the largest slices whose LDS still holds both tiles of a unit in one reduction round (7 x 3 at 3 row blocks
  // reduced a tile at a time and measured 63.8 against 58.1 us on gate/up at 48 rows, 7 x 2 at 4 row blocks 48.7
  // against 46.7 us on the down at 64).  S slices of `per` code steps, units of two packed tiles, about one workgroup
  // per CU.  S > 1: the slabs are merged by a second launch (k_w8_rows_merge), one small workgroup per (tile, row
  // block)
  const int RB = (M + 15) / 16;
  const int NW = RB == 4 ? 6 : 7, KPW = RB == 2 ? 4 : 2;
  const int S = (KK + NW * KPW - 1) / (NW * KPW), per = (KK + S - 1) / S;
  const int pairs = (ntiles + 1) / 2;
  const int per_split = w8_cus() / S < 1 ? 1 : w8_cus() / S;
  const int G = pairs < per_split ? pairs : per_split;
  if (S > 1) {
    const long long need = (long long)S * RB * 16 * ntiles * 16;
    FO_REQUIRE(ws && need <= ws_floats,
               "fo_gemm_w8_rows: K=%d splits over %d workgroups: split-K workspace too small (%lld floats needed, "
               "%lld given)", K, S, need, ws ? ws_floats : 0ll);
  }
  (void)counters;
  if (sgroups) *sgroups = units;
  const dim3 grid(G, S), block(NW * 64);
#define FO_W8_ROWS(NW_, KPW_, RB_)                                                                         \
  do {                                                                                                     \
    if (swiglu) hipLaunchKernelGGL((k_w8_rows<NW_, KPW_, RB_, true>), grid, block, 0, stream, a, S, per, ws); \
    else hipLaunchKernelGGL((k_w8_rows<NW_, KPW_, RB_, false>), grid, block, 0, stream, a, S, per, ws);    \
  } while (0)
  if (RB == 2) FO_W8_ROWS(7, 4, 2);
  else if (RB == 3) FO_W8_ROWS(7, 2, 3);
  else FO_W8_ROWS(6, 2, 4);
#undef FO_W8_ROWS
  if (S > 1) {
    const int rc = fo::check_launch("fo_gemm_w8_rows");
    if (rc) return rc;
    launch_merge<true>(a, swiglu, units, RB, S, ws, stream);
  }
  fo::count_launch(FO_L_GEMM_W8_ROWS);
  return fo::check_launch("fo_gemm_w8_rows");
}

int fo_gemm_w8_rows128(const float* X, int ldx, int M, int K, const void* Q, const float* scale, int ntiles, int N,
                       int swiglu, float* Y, int ldy, int residual, float* ws, long long ws_floats, int* counters,
                       const float* rstats, int rgroups, float eps, float* sout, const float* gnext, float* yg,
                       int* sgroups, hipStream_t stream) {
  W8Args a;
  int units;
  if (const int rc = w8_args("fo_gemm_w8_rows128", 65, 128,
                             "this FP8 stream serves 65 <= M <= 128 (fo_gemm_w8 serves M <= 16, fo_gemm_w8_rows 17..64, "
                             "more than 128 rows run the bf16 image)",
                             X, ldx, M, K, Q, scale, ntiles, N, swiglu, Y, ldy, residual, rstats, rgroups, eps, sout,
                             gnext, yg, a, units))
    return rc;
  const int KK = a.KK;
  // The plan of k_gemm_rows (fo_gemm.hip plan_rows).  A workgroup's X over its K slice (512 B per column at 128 rows)
  // passes through its CU beside its codes (16 B per tile and column), so the tiles per workgroup are as many as the
  // accumulators and the LDS ring allow and K is split until the grid is about one workgroup per CU: SwiGLU K thirds
  // of up to 15 (gate, up) pairs (the Qwen2 gate/up: 3 x 85 workgroups of 28 tiles), plain 14 or 16 tiles and up to
  // 16 slices (the Qwen2 down: 16 x 16 workgroups of 14 tiles x 18.5 code steps).  Never more slices than code steps.
  const int RB = (M + 15) / 16, cus = w8_cus();
  int tiles_per, G, S;
  if (swiglu) {
    S = KK < 3 ? KK : 3;
    int per = (S * units + cus - 1) / cus;
    per = per < 1 ? 1 : (per > 15 ? 15 : per);
    tiles_per = 2 * per;
    G = (units + per - 1) / per;
  } else {
    tiles_per = ntiles % 14 == 0 ? 14 : 16;
    G = (ntiles + tiles_per - 1) / tiles_per;
    S = cus / G;
    S = S < 1 ? 1 : (S > 16 ? 16 : S);
    S = S > KK ? KK : S;
  }
  const long long need = (long long)S * RB * 16 * ntiles * 16;
  FO_REQUIRE(ws && need <= ws_floats,
             "fo_gemm_w8_rows128: K=%d in %d slices: split-K workspace too small (%lld floats needed, %lld given)", K,
             S, need, ws ? ws_floats : 0ll);
  (void)counters;
  if (sgroups) *sgroups = units;
  const int total = S * G;
  const dim3 grid(8 * ((total + 7) / 8)), block(512);
  // ring depth: two code steps ahead where 3 slots of (tiles + 32) KiB fit the LDS, one (k_gemm_rows's two k-steps)
  // at the gate/up's 28 tiles
#define FO_W8_ROWS128(NTC_, D_) \
  hipLaunchKernelGGL((k_w8_rows128<NTC_, D_>), grid, block, 0, stream, a, S, G, tiles_per, ws)
  if (tiles_per > 20) FO_W8_ROWS128(30, 1);
  else if (tiles_per > 16) FO_W8_ROWS128(20, 2);
  else if (tiles_per == 14) FO_W8_ROWS128(14, 2);
  else FO_W8_ROWS128(16, 2);
#undef FO_W8_ROWS128
  const int rc = fo::check_launch("fo_gemm_w8_rows128");
  if (rc) return rc;
  launch_merge<true>(a, swiglu, units, RB, S, ws, stream);
  fo::count_launch(FO_L_GEMM_W8_ROWS128);
  return fo::check_launch("fo_gemm_w8_rows128 (merge)");
}

}  // extern "C"
