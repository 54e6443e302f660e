// The weight-stream GEMMs over quantised codes, once for every format: the argument block, the X split, the epilogue,
// the consumer's rstd, the five kernel forms (k_wq, k_wq_qkv, k_wq_sk, k_wq_xs, k_wq_rows), the merge of the row
// streams' split-K slabs, and the host side (argument checks, dispatch, plans).  What differs per format is a struct F
// in the format's file (fo_gemm_w8.hip: Fp8, e4m3 codes with a scale per output column; fo_gemm_w4.hip: Mxfp4 and
// fo_gemm_w6.hip: Mxfp6, codes whose E8M0 block scale is applied in the decode):
//   COLS, FR, STEP, SCALED   columns / MFMA fragments / bytes of one code step of a tile; a column scale in the epilogue
//   Code, zero(), Srd, srd(), load()   one lane's register image of one code step (an MX format's scale dword inside
//                            it), its all-zero value, the buffer descriptors (exactly the codes and the scale bytes: a
//                            step past them loads zero codes under a zero scale byte) and the load of step tile * KK + k
//   decode(q, lane, w[FR])   that image to the FR B fragments of the step's MFMAs
//   xcol(g, j), xblock(g, j) the register-resident forms: the X column, from the wave's first code step, of lane group
//                            g's A fragment j, and the start of the 32-column block that decides whether it is past K
//   accumulate<NT, U>()      the streaming forms' inner loop, U code steps in flight
//   U_PAIR, U_PLAIN, U_SK    that depth per form; XS / XS_ALT / XS_ENV / XS_ALT_ARG the xs wave shapes and the A/B
//                            switch, XS_REREAD_LO whether k_wq_xs re-reads its lo fragments from LDS per tile;
//   ROWS[RB - 2][swiglu]     the rows form's (NW, KPW)
//   GEMM, QUANT, PAIR_CHECK, count()   the host's words and launch counters
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include "fo_common.h"

namespace fo {
// the launch counters of the lm_head streams (fo_gemm_head_counts, fo_capi.hip): slot 0 fo_gemm_w8_head, slot 1
// fo_gemm_w4_head.  Counters of their own: these kernels have no FoLaunchKind.
void count_head(int slot);
// the launch counters of the quantised q|k|v streams (fo_gemm_qkv_quant_counts, fo_capi.hip): slot 0
// fo_gemm_w8_qkv_rope, slot 1 fo_gemm_w4_qkv_rope
void count_qkv_quant(int slot);
}  // namespace fo

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

struct WqArgs {
  const float* X;
  const void* Q;       // codes in packed order
  const float* scale;  // [ntiles][16], packed tile order (an MX format: the E8M0 block-scale bytes, read by the decode)
  float* Y;
  int ldx, ldy;
  int M, K, N;         // N: logical output columns (after SwiGLU pairing)
  int ntiles;          // packed 16-column tiles in Q
  int KK;              // code steps per tile: ceil(K / F::COLS)
  int residual;
  // the RMSNorm split across two GEMMs, as fo_gemm_rms (fo_gemm.hip GemmArgs)
  float* sout;
  const float* gnext;
  float* yg;
  const float* rstats;
  int rgroups;
  float reps;
};

// The fused q|k|v projection's epilogue on the code streams (fo_gemm_w8_qkv_rope / fo_gemm_w4_qkv_rope): what
// fo_gemm_qkv_rope_kv's GemmArgs carry in their r* fields (fo_gemm.hip), beside WqArgs.
struct QkvRopeArgs {
  const float* bias;   // [N] or NULL
  const int* pos;      // [M] the token's position
  const int* slot;     // [M] the token's slot of the paged cache
  const float* cos_t;  // [pos][hd/2]
  const float* sin_t;
  float* q_out;        // [M][H * hd]
  void* kc;            // one layer's pages [page][KVH][PS][hd]: fp32, or bf16 elements (kv16)
  void* vc;
  int H, KVH, hd, PS;
  int kv16;            // the cache holds bf16: K / V stored as f2bf(x)
  int kvb;             // an fp32 cache takes the bf16 value of K / V (fo_set_kv_bf16)
};

// Elements o and o + half of the paged cache `base`, as fo_gemm.hip's kv_store
__device__ __forceinline__ void wq_kv_store(const QkvRopeArgs& r, void* base, size_t o, int half, float x1, float x2) {
  if (r.kv16) {
    bf16_t* d = reinterpret_cast<bf16_t*>(base) + o;
    d[0] = f2bf(x1);
    d[half] = f2bf(x2);
  } else {
    float* d = reinterpret_cast<float*>(base) + o;
    d[0] = r.kvb ? bf2f(f2bf(x1)) : x1;
    d[half] = r.kvb ? bf2f(f2bf(x2)) : x2;
  }
}

// Output elements (row rr, logical columns n and n + hd/2) of rope tile pair P, n = rope_col(P, c): x1 / x2 are the
// fp32 sums of packed tiles 2P / 2P + 1.  In this order: the FP8 column scales (SCALED; the MX formats' sums carry their
// block scales already), the consumer's rstd, the bias, rotate_half RoPE at pos[rr] for q and k heads, the store: q to
// q_out, K and V to the paged cache at slot[rr].  Rows >= M (computed from a clamped row) are never stored.
template <bool SCALED>
__device__ __forceinline__ void wq_rope_epilogue(const WqArgs& a, const QkvRopeArgs& r, int P, int rr, int c, float x1,
                                                 float x2, const float* rstd_s) {
  if (rr >= a.M) return;
  const int hd = r.hd, half = hd >> 1, per = hd >> 5;   // per: tile pairs per head
  const int h = P / per, i = (P - h * per) * 16 + c;
  const int n = h * hd + i;
  if constexpr (SCALED) {
    x1 *= a.scale[(2 * P) * 16 + c];
    x2 *= a.scale[(2 * P + 1) * 16 + c];
  }
  if (a.rstats) {
    x1 *= rstd_s[rr];
    x2 *= rstd_s[rr];
  }
  if (r.bias) {
    x1 += r.bias[n];
    x2 += r.bias[n + half];
  }
  if (h < r.H + r.KVH) {
    const int p = r.pos[rr];
    const float cs = r.cos_t[(size_t)p * half + i], sn = r.sin_t[(size_t)p * half + i];
    const float o1 = x1 * cs - x2 * sn, o2 = x2 * cs + x1 * sn;
    x1 = o1;
    x2 = o2;
  }
  if (h < r.H) {
    float* d = r.q_out + (size_t)rr * r.H * hd + (size_t)h * hd;
    d[i] = x1;
    d[i + half] = x2;
    return;
  }
  const int sl = r.slot[rr];
  const int page = sl / r.PS, off = sl - page * r.PS;
  const bool isk = h < r.H + r.KVH;
  const int kvh = h - r.H - (isk ? 0 : r.KVH);
  wq_kv_store(r, isk ? r.kc : r.vc, (((size_t)page * r.KVH + kvh) * r.PS + off) * hd + i, half, x1, x2);
}

__device__ __forceinline__ void split8(const float4 p0, const float4 p1, bf16x8& hi, bf16x8& lo) {
  const float f[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const __bf16 h = (__bf16)f[i];
    hi[i] = h;
    lo[i] = (__bf16)(f[i] - (float)h);
  }
}

// Output element (row rr, column c) of unit u, thread e = 16 rr + c of the first 256: x1 / x2 are the fp32 sums of
// the unit's (gate, up) tiles (SW) or of its one tile.  The column scale first (SCALED; the MX formats' sums carry their
// block scales already), then the consumer's rstd, SwiGLU, the residual and the store; a producer also writes
// yg = y * gamma_next and the row's sum of squares over the unit's 16 columns.  Rows >= M (computed from a clamped
// row) are neither stored nor summed.
template <bool SW, bool SCALED>
__device__ __forceinline__ void wq_epilogue(const WqArgs& a, int u, int groups, int rr, int c, float x1, float x2,
                                            const float* rstd_s) {
  const int n = u * 16 + c;
  const bool live = rr < a.M && n < a.N;
  float y = 0.f;
  if (live) {
    if constexpr (SCALED) {
      if constexpr (SW) {
        x1 *= a.scale[(2 * u) * 16 + c];
        x2 *= a.scale[(2 * u + 1) * 16 + c];
      } else {
        x1 *= a.scale[n];
      }
    }
    if (a.rstats) {
      x1 *= rstd_s[rr];
      x2 *= rstd_s[rr];
    }
    y = SW ? x1 / (1.f + expf(-x1)) * x2 : x1;
    const size_t o = (size_t)rr * a.ldy + n;
    if (a.residual) y += a.Y[o];
    a.Y[o] = y;
    if (a.yg) a.yg[o] = y * a.gnext[n];
  }
  if constexpr (!SW) {
    if (a.sout) {   // (uniform; the row's 16 columns are one 16-lane row of the wave)
      float sq = y * y;
      sq += lane_xor<8>(sq);
      sq += lane_xor<4>(sq);
      sq += lane_xor<2>(sq);
      sq += lane_xor<1>(sq);
      if (c == 0 && rr < a.M) a.sout[(size_t)rr * groups + u] = sq;
    }
  }
}

// The consumer's rstd of rows [r0, r0 + n) into rstd_s[row], a row per wave of NW: the row's statistics summed
// lane-strided, then across the wave.  Rows >= M take the last row's (computed, never stored).
template <int NW>
__device__ __forceinline__ void wq_rstd(const WqArgs& a, float* rstd_s, int wave, int lane, int r0 = 0, int n = 16) {
  for (int r = wave; r < n; r += NW) {
    const int rr = r0 + r, m = min(rr, a.M - 1);
    float v = 0.f;
    for (int j = lane; j < a.rgroups; j += 64) v += a.rstats[(size_t)m * a.rgroups + j];
    v = wave_sum(v);
    if (lane == 0) rstd_s[rr] = rsqrtf(v / (float)a.K + a.reps);
  }
}

// One wave's accumulator tile (a lane holds rows 4 (lane >> 4) .. + 4 of column lane & 15) into a padded LDS tile
template <typename Tile>
__device__ __forceinline__ void wq_store_tile(Tile& tile, const f32x4 acc, int lane, int r0 = 0) {
#pragma unroll
  for (int i = 0; i < 4; ++i) tile[r0 + 4 * (lane >> 4) + i][lane & 15] = acc[i];
}

// Element (t, rr, c) of the waves' partial tiles in `part`, summed in wave order
template <int NW, int T, int R>
__device__ __forceinline__ float wq_sum_waves(const float (&part)[NW][T][R][17], int t, int rr, int c) {
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) s += part[w][t][rr][c];
  return s;
}

// The descriptors and the scale load the MX formats share: scale bytes [tile][K128][16 rows][4], a lane reading its
// row's dword (which byte it uses is the format's: the decode takes it)
struct WqMxSrd {
  __amdgpu_buffer_rsrc_t q, s;
};
template <int STEP>
__device__ __forceinline__ WqMxSrd wq_mx_srd(const WqArgs& a) {
  return WqMxSrd{rsrc_of(a.Q, a.ntiles * a.KK * STEP), rsrc_of(a.scale, a.ntiles * a.KK * 64)};
}
__device__ __forceinline__ unsigned wq_mx_scale(const WqMxSrd& d, int lane, int step) {
  return __builtin_amdgcn_raw_buffer_load_b32(d.s, (lane & 15) * 4, step * 64, 0);
}

// What the streaming forms share: the T packed tiles from tile0 over the code steps [k_lo, k_lo + k_n), wave w taking
// [k_n w / NW, k_n (w + 1) / NW) of them with U (per tile) in flight, into part[w] (and the consumer's rstd into
// rstd_s); returns behind the barrier.
template <typename F, int NW, int T, int U>
__device__ __forceinline__ void wq_stream_tiles(const WqArgs& a, int tile0, int k_lo, int k_n,
                                                float (&part)[NW][T][16][17], float* rstd_s) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const typename F::Srd d = F::srd(a);
  const int kb = k_lo + (int)((long)k_n * wave / NW), ke = k_lo + (int)((long)k_n * (wave + 1) / NW);
  const int row = min(lane & 15, a.M - 1);
  const float* xp = a.X + (size_t)row * a.ldx + 8 * (lane >> 4);
  if (a.rstats) wq_rstd<NW>(a, rstd_s, wave, lane);
  f32x4 acc[T];
  F::template accumulate<T, U>(a, d, xp, lane, tile0, kb, ke, acc);
#pragma unroll
  for (int t = 0; t < T; ++t) wq_store_tile(part[wave][t], acc[t], lane);
  __syncthreads();
}

// ---- general form: workgroup u = output tile u (SW: the (gate, up) pair 2u, 2u + 1); wave w takes the code steps
// [KK w / NW, KK (w + 1) / NW), F::U_PAIR / F::U_PLAIN of them (per tile) in flight
template <typename F, int NW, bool SW>
__global__ __launch_bounds__(NW * 64) void k_wq(WqArgs a) {
  constexpr int T = SW ? 2 : 1;
  __shared__ float part[NW][T][16][17];
  __shared__ float rstd_s[16];
  const int u = blockIdx.x;
  wq_stream_tiles<F, NW, T, (SW ? F::U_PAIR : F::U_PLAIN)>(a, T * u, 0, a.KK, part, rstd_s);
  const int e = threadIdx.x;
  if (e < 256) {
    const int rr = e >> 4, c = e & 15;
    wq_epilogue<SW, F::SCALED>(a, u, gridDim.x, rr, c, wq_sum_waves(part, 0, rr, c), wq_sum_waves(part, T - 1, rr, c),
                               rstd_s);
  }
}

// ---- the fused q|k|v projection (fo_gemm_w8_qkv_rope / fo_gemm_w4_qkv_rope): k_wq's pair form with the RoPE +
// paged-KV epilogue in place of SwiGLU.  Workgroup P = rope tile pair P (packed tiles 2P, 2P + 1: columns (i, i + hd/2)
// of one head); the waves split the code steps as in k_wq and the cross-wave sum runs in wave order.  No workspace, no
// tickets.
template <typename F, int NW>
__global__ __launch_bounds__(NW * 64) void k_wq_qkv(WqArgs a, QkvRopeArgs r) {
  __shared__ float part[NW][2][16][17];
  __shared__ float rstd_s[16];
  const int P = blockIdx.x;
  wq_stream_tiles<F, NW, 2, F::U_PAIR>(a, 2 * P, 0, a.KK, part, rstd_s);
  const int e = threadIdx.x;
  if (e < 256) {
    const int rr = e >> 4, c = e & 15;
    wq_rope_epilogue<F::SCALED>(a, r, P, rr, c, wq_sum_waves(part, 0, rr, c), wq_sum_waves(part, 1, rr, c), rstd_s);
  }
}

// ---- long-K plain form: workgroup (tg, sp) = tiles NT tg .. + NT over the sp-th of S slices of the code steps, the
// slice split over the waves as in k_wq.  ws: S slabs of [16][groups * NT * 16] partial sums; counters: one zeroed
// ticket per tile group, left zeroed.  The hand-off is fo_common.h's (st_wt / ld_sc1): no fences, no waiting; the last
// split to arrive sums every split's partial in split order.
template <typename F, int NW, int NT>
__global__ __launch_bounds__(NW * 64) void k_wq_sk(WqArgs a, int S, float* ws, int* counters) {
  __shared__ float part[NW][NT][16][17];
  __shared__ float red[NT][16][17];
  __shared__ float rstd_s[16];
  __shared__ int last_s;
  const int tg = blockIdx.x, sp = blockIdx.y;
  const int k_lo = (int)((long)a.KK * sp / S), k_n = (int)((long)a.KK * (sp + 1) / S) - k_lo;
  wq_stream_tiles<F, NW, NT, F::U_SK>(a, NT * tg, k_lo, k_n, part, rstd_s);
  constexpr int NE = NT * 256, NTH = NW * 64;
  for (int e = threadIdx.x; e < NE; e += NTH) {
    const int t = e >> 8, rr = (e >> 4) & 15, c = e & 15;
    red[t][rr][c] = wq_sum_waves(part, t, rr, c);
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
      if (tg * NT + t < units) wq_epilogue<false, F::SCALED>(a, tg * NT + t, units, rr, c, red[t][rr][c], 0.f, rstd_s);
  }
}

// ---- X-stationary persistent form, as k_gemm_xs (fo_gemm.hip): the SwiGLU pair, K = NW * KPW * F::COLS (3584).  X hi
// in registers, lo in LDS, units dealt evenly to at most one workgroup per CU, the next unit's codes (and scales)
// issued before the current one is reduced, a fixed-order cross-wave reduction.
// SW = false (the fo_gemm_w*_head entries): the plain form.  A unit is two adjacent plain tiles 2u, 2u + 1 (the second
// of an odd count's last unit lies past the descriptors and loads zero codes; it is never stored), each with the plain
// epilogue: the column scale (F::SCALED) and the store, no residual, no statistics (NW * 64 >= 512: a tile per 256
// threads).
template <typename F, int NW, int KPW, bool SW = true>
__global__ __launch_bounds__(NW * 64) void k_wq_xs(WqArgs a, int units) {
  static_assert(SW || NW >= 8, "k_wq_xs: the plain epilogue takes 512 threads");
  constexpr int FR = F::FR, KK = NW * KPW;
  __shared__ bf16x8 xlo[NW][FR * KPW][64];
  __shared__ float part[NW][2][16][17];
  __shared__ float rstd_s[16];
  // (the wave index through readfirstlane: the code steps' offsets are then scalars the buffer loads take as they are)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ub = (int)((long)units * blockIdx.x / gridDim.x);
  const int ue = (int)((long)units * (blockIdx.x + 1) / gridDim.x);
  const typename F::Srd d = F::srd(a);
  typename F::Code q0[KPW], q1[KPW];
  auto issue = [&](typename F::Code (&q)[KPW], int tile) {
#pragma unroll
    for (int j = 0; j < KPW; ++j) q[j] = F::load(d, lane, tile * KK + wave * KPW + j);
  };
  issue(q0, ub < ue ? 2 * ub : a.ntiles);
  issue(q1, ub < ue ? 2 * ub + 1 : a.ntiles);
  // X slice (hi in registers, lo in LDS); rows >= M clamp to the last row (computed, never stored)
  bf16x8 xh[FR * KPW];
  {
    const int row = min(lane & 15, a.M - 1);
    const float* xp = a.X + (size_t)row * a.ldx + (size_t)wave * KPW * F::COLS;
#pragma unroll
    for (int j = 0; j < FR * KPW; ++j) {
      const float4* p = reinterpret_cast<const float4*>(xp + F::xcol(lane >> 4, j));
      bf16x8 lo;
      split8(p[0], p[1], xh[j], lo);
      xlo[wave][j][lane] = lo;
    }
  }
  if constexpr (SW) {
    if (a.rstats) wq_rstd<NW>(a, rstd_s, wave, lane);
  }
  auto compute = [&](typename F::Code (&q)[KPW]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // (F::XS_REREAD_LO: the lo fragments are re-read from LDS per tile, an opaque lane index keeping the compiler from
    // hoisting the loop-invariant reads into FR KPW more live registers)
    int ln = lane;
    if constexpr (F::XS_REREAD_LO) asm volatile("" : "+v"(ln));
#pragma unroll
    for (int j = 0; j < KPW; ++j) {
      bf16x8 w[FR];
      F::decode(q[j], lane, w);
#pragma unroll
      for (int h = 0; h < FR; ++h) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[FR * j + h], w[h], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xlo[wave][FR * j + h][ln], w[h], acc, 0, 0, 0);
      }
    }
    return acc;
  };
  for (int u = ub; u < ue; ++u) {
    // the next unit's codes are issued unconditionally; past the last unit they address tile `ntiles`, beyond the
    // descriptors' range, which the hardware drops without touching memory
    const int nxt = u + 1 < ue ? 2 * (u + 1) : a.ntiles;
    const f32x4 c0 = compute(q0);
    issue(q0, nxt);
    const f32x4 c1 = compute(q1);
    issue(q1, nxt + (u + 1 < ue ? 1 : 0));
    __syncthreads();  // the previous unit's epilogue has read part[]
    wq_store_tile(part[wave][0], c0, lane);
    wq_store_tile(part[wave][1], c1, lane);
    __syncthreads();
    const int e = threadIdx.x;
    if constexpr (SW) {
      if (e < 256) {
        const int rr = e >> 4, c = e & 15;
        wq_epilogue<true, F::SCALED>(a, u, 0, rr, c, wq_sum_waves(part, 0, rr, c), wq_sum_waves(part, 1, rr, c),
                                     rstd_s);
      }
    } else if (e < 512) {
      const int t = e >> 8, rr = (e >> 4) & 15, c = e & 15;
      const float x1 = wq_sum_waves(part, t, rr, c);
      if (2 * u + t < a.ntiles) wq_epilogue<false, F::SCALED>(a, 2 * u + t, 0, rr, c, x1, 0.f, rstd_s);
    }
  }
}

// ---- 17..64 rows (RB = 2..4 row blocks of 16): X-stationary with K split over workgroups, k_gemm_xsk's design
// (fo_gemm.hip) on the codes.  Workgroup (g, sp): the sp-th of S slices of the code steps for units [ub, ue) of
// column group g; a unit is a packed tile pair (the (gate, up) pair, or two adjacent plain tiles: the second of an
// odd count's last pair lies past the descriptors and loads zero codes).  Wave w owns KPW code steps of the slice:
// their X fragments of all RB row blocks (F::xcol) are split once (hi in VGPRs, lo in its LDS region; a fragment whose
// 32-column block, F::xblock, lies at or past K -- K % F::COLS != 0, the last code step -- holds zeros and reads no X:
// X may end at the last row's column K), each code step's image is decoded once per unit and feeds RB x (hi, lo) MFMAs
// per fragment, the next two units' codes in flight meanwhile.  Per unit the NW partial tiles are summed through LDS
// in wave order (both tiles in one round where the LDS allows).  S == 1: the epilogue follows.  S > 1: the sums are
// stored as split sp's slab of `ws` ([S][RB * 16][ntiles * 16] floats) and k_wq_rows_merge, the next launch, sums the
// slabs in split order and runs the epilogue.
template <typename F, int NW, int KPW, int RB, bool SW>
__global__ __launch_bounds__(NW * 64) void k_wq_rows(WqArgs a, int S, int per, float* ws) {
  constexpr int FR = F::FR, ROWS = RB * 16, NTH = NW * 64, NE = ROWS * 16, EPT = (NE + NTH - 1) / NTH;
  constexpr int PT = (NW * RB * FR * KPW * 1024 + NW * 2 * ROWS * 17 * 4 + 512 <= 160 * 1024) ? 2 : 1;
  __shared__ bf16x8 xlo[NW][RB][FR * KPW][64];
  __shared__ float part[NW][PT][ROWS][17];
  __shared__ float rstd_s[ROWS];
  // (the wave index through readfirstlane: the code steps' offsets are then scalars the buffer loads take as they are)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int G = gridDim.x, g = blockIdx.x, sp = blockIdx.y;
  const int units = (a.ntiles + 1) >> 1, tiles = (a.N + 15) / 16;   // (tiles: output tiles, the statistics' groups)
  const int ub = (int)((long)units * g / G), ue = (int)((long)units * (g + 1) / G);
  const typename F::Srd d = F::srd(a);
  // this wave's code steps: [k0, k0 + nj) inside the slice [sp * per, (sp + 1) * per) and inside KK (wave-uniform)
  const int k0 = sp * per + wave * KPW;
  const int nj = max(0, min(KPW, min(a.KK, (sp + 1) * per) - k0));
  typename F::Code q[2][2][KPW];
  auto issue = [&](typename F::Code (&qq)[2][KPW], int u) {   // u >= ue: past the workgroup's range, no load issued
    if (u < ue) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < KPW; ++j)
          if (j < nj) qq[t][j] = F::load(d, lane, (2 * u + t) * a.KK + k0 + j);
    }
  };
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < KPW; ++j) q[b][t][j] = F::zero();   // code steps past the slice: zero codes
  issue(q[0], ub);
  issue(q[1], ub + 1);
  bf16x8 zero;
#pragma unroll
  for (int i = 0; i < 8; ++i) zero[i] = (__bf16)0.f;
  bf16x8 xh[RB][FR * KPW];
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const int row = min(r * 16 + (lane & 15), a.M - 1);   // rows >= M: computed, never stored or summed
    const float* xp = a.X + (size_t)row * a.ldx + (size_t)k0 * F::COLS;
#pragma unroll
    for (int j = 0; j < FR * KPW; ++j) {
      bf16x8 hi = zero, lo = zero;
      if (j / FR < nj && k0 * F::COLS + F::xblock(lane >> 4, j) < a.K) {
        const float4* p = reinterpret_cast<const float4*>(xp + F::xcol(lane >> 4, j));
        split8(p[0], p[1], hi, lo);
      }
      xh[r][j] = hi;
      xlo[wave][r][j][lane] = lo;
    }
  }
  if (S == 1) {   // the consumer's rstd of every row (rows >= M from the clamped row)
    if (a.rstats) wq_rstd<NW>(a, rstd_s, wave, lane, 0, ROWS);
    __syncthreads();
  }
  const int Ncols = a.ntiles * 16;
  float* slab = ws + (size_t)sp * ROWS * Ncols;
  auto unit = [&](typename F::Code (&qq)[2][KPW], int u) {
    float v[2][EPT];
    // (the lo fragments are re-read from LDS per unit, as in k_wq_xs: an opaque lane index keeps the compiler from
    // hoisting the loop-invariant reads into RB * FR KPW more live registers, which spilled MXFP6 at 2 row blocks)
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
          bf16x8 w[FR];
          F::decode(qq[t0 + p][j], lane, w);
#pragma unroll
          for (int h = 0; h < FR; ++h)
#pragma unroll
            for (int r = 0; r < RB; ++r) {
              acc[p][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[r][FR * j + h], w[h], acc[p][r], 0, 0, 0);
              acc[p][r] =
                  __builtin_amdgcn_mfma_f32_16x16x32_bf16(xlo[wave][r][FR * j + h][ln], w[h], acc[p][r], 0, 0, 0);
            }
        }
      }
      if (t0 + PT == 2) issue(qq, u + 2);   // (the unit's codes are decoded: its buffer takes the unit after next)
      __syncthreads();  // the previous reduction has read part[]
#pragma unroll
      for (int p = 0; p < PT; ++p)
#pragma unroll
        for (int r = 0; r < RB; ++r) wq_store_tile(part[wave][p], acc[p][r], lane, r * 16);
      __syncthreads();
#pragma unroll
      for (int p = 0; p < PT; ++p)
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
          const int e = threadIdx.x + i * NTH;
          float s = 0.f;
          if (e < NE) {
            s = wq_sum_waves(part, p, e >> 4, e & 15);
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
          wq_epilogue<true, F::SCALED>(a, u, tiles, rr, c, v[0][i], v[1][i], rstd_s);
        } else {
          wq_epilogue<false, F::SCALED>(a, 2 * u, tiles, rr, c, v[0][i], 0.f, rstd_s);
          if (2 * u + 1 < a.ntiles) wq_epilogue<false, F::SCALED>(a, 2 * u + 1, tiles, rr, c, v[1][i], 0.f, rstd_s);
        }
      }
    }
  };
  for (int u = ub; u < ue; u += 2) {   // (workgroup-uniform: every wave reaches unit's barriers)
    unit(q[0], u);
    if (u + 1 < ue) unit(q[1], u + 1);
  }
}

// The merge of the row-stream kernels' slabs (k_wq_rows, k_w8_rows128): workgroup (u, rb) = output tile u
// (SW: the (gate, up) pair) x row block rb, thread 16 rr + c one element: every split's partial summed in split order
// (8 loads in flight; a missing split adds 0), then the epilogue (SCALED: with the FP8 column scale).
template <bool SW, bool SCALED>
__global__ __launch_bounds__(256) void k_wq_rows_merge(WqArgs a, int S, const float* ws, int rows) {
  constexpr int T = SW ? 2 : 1;
  __shared__ float rstd_s[128];   // (indexed by the row: up to k_w8_rows128's 8 row blocks)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = blockIdx.x, rb = blockIdx.y;
  if (a.rstats) {
    wq_rstd<4>(a, rstd_s, wave, lane, rb * 16, 16);
    __syncthreads();
  }
  const int rr = rb * 16 + (threadIdx.x >> 4), c = threadIdx.x & 15;
  const int Ncols = a.ntiles * 16;
  const size_t sl = (size_t)rows * Ncols;
  float x[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const float* p0 = ws + (size_t)rr * Ncols + (T * u + t) * 16 + c;
    float s = 0.f;
    for (int s0 = 0; s0 < S; s0 += 8) {
      float p[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) p[k] = s0 + k < S ? p0[(s0 + k) * sl] : 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) s += p[k];
    }
    x[t] = s;
  }
  wq_epilogue<SW, SCALED>(a, u, gridDim.x, rr, c, x[0], x[T - 1], rstd_s);
}

// k_wq_rows_merge over the S slabs of RB row blocks in `ws`
template <bool SCALED>
void launch_merge(const WqArgs& a, int swiglu, int units, int RB, int S, const float* ws, hipStream_t stream) {
  if (swiglu)
    hipLaunchKernelGGL((k_wq_rows_merge<true, SCALED>), dim3(units, RB), dim3(256), 0, stream, a, S, ws, RB * 16);
  else
    hipLaunchKernelGGL((k_wq_rows_merge<false, SCALED>), dim3(units, RB), dim3(256), 0, stream, a, S, ws, RB * 16);
}

// ---- the host side.  An entry's arguments as include/fo_hip.h lists them, and its name, row band and what its
// refusal says of the band
struct WqCall {
  const float* X;
  int ldx, M, K;
  const void* Q;
  const void* scale;
  int ntiles, N, swiglu;
  float* Y;
  int ldy, residual;
  float* ws;
  long long ws_floats;
  int* counters;
  const float* rstats;
  int rgroups;
  float eps;
  float* sout;
  const float* gnext;
  float* yg;
  int* sgroups;
  hipStream_t stream;
};
// (an MLP entry's arguments, in WqCall's order)
#define FO_WQ_CALL                                                                                                    \
  WqCall {                                                                                                            \
    X, ldx, M, K, Q, scale, ntiles, N, swiglu, Y, ldy, residual, ws, ws_floats, counters, rstats, rgroups, eps, sout, \
        gnext, yg, sgroups, stream                                                                                    \
  }
struct WqEntry {
  const char* fn;
  int m_lo, m_hi;
  const char* serves;
};
enum WqForm { WQ_GENERAL, WQ_XS, WQ_SK, WQ_HEAD, WQ_QKV, WQ_ROWS };   // what F::count counts
struct WqShape {
  int nw, kpw;   // waves x code steps per wave
};

inline int wq_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus = n;
  }
  return cus;
}

// fo::check_launch under the entry's name and the form's suffix
inline int wq_check(const char* fn, const char* form = "") {
  if (hipPeekAtLastError() == hipSuccess) return 0;
  char what[96];
  snprintf(what, sizeof(what), "%s%s", fn, form);
  return fo::check_launch(what);
}

// What the GEMM entries share: the checks of everything but the workspace (all before the entry's first HIP call),
// then WqArgs (with KK) and the output tile count.  (F::PAIR_CHECK: the MX entries refuse an odd SwiGLU tile count in
// words of its own; the FP8 entries' tile-count check covers it, and fo_gemm_w8 says it first.)
template <typename F>
int wq_args(const WqEntry& en, const WqCall& c, WqArgs& a, int& units) {
  const char* fn = en.fn;
  const int M = c.M, K = c.K, N = c.N, ntiles = c.ntiles, swiglu = c.swiglu;
  FO_REQUIRE(M > 0 && N > 0 && K > 0, "%s: bad shape M=%d N=%d K=%d", fn, M, N, K);
  FO_REQUIRE(M >= en.m_lo && M <= en.m_hi, "%s: M=%d rows, %s", fn, M, en.serves);
  FO_REQUIRE((K & 31) == 0, "%s: K=%d must be a multiple of 32", fn, K);
  FO_REQUIRE(c.X && c.Q && c.Y, "%s: NULL X, Q or Y", fn);
  FO_REQUIRE(c.scale, "%s: NULL scale (%s)", fn, F::QUANT);
  FO_REQUIRE(c.ldx >= K && (c.ldx & 3) == 0 && ((unsigned long long)c.X & 15) == 0,
             "%s: X needs ldx=%d >= K=%d, ldx %% 4 == 0 and 16-byte alignment", fn, c.ldx, K);
  FO_REQUIRE(c.ldy >= N, "%s: ldy=%d < N=%d", fn, c.ldy, N);
  units = (N + 15) / 16;
  FO_REQUIRE(!F::PAIR_CHECK || !swiglu || (ntiles & 1) == 0,
             "%s: swiglu with an odd ntiles=%d (gate/up tiles come in pairs)", fn, ntiles);
  // ntiles is the extent of Q and scale (the descriptors' range): (gate, up) pairs for SwiGLU
  FO_REQUIRE(ntiles == (swiglu ? 2 : 1) * units, "%s: ntiles=%d packed tiles for N=%d%s", fn, ntiles, N,
             swiglu ? " SwiGLU columns" : " columns");
  FO_REQUIRE(!c.rstats || c.rgroups > 0, "%s: rstats without rgroups", fn);
  FO_REQUIRE(!c.sout || (!swiglu && (!c.yg || c.gnext)), "%s: sout needs a non-SwiGLU launch, yg needs gnext", fn);
  FO_REQUIRE(c.sout || !c.yg, "%s: yg comes with sout", fn);
  FO_REQUIRE(!(swiglu && c.residual), "%s: swiglu with residual unsupported", fn);
  const int KK = (K + F::COLS - 1) / F::COLS;
  FO_REQUIRE((long long)(ntiles + 4) * KK * F::STEP < (1ll << 31), "%s: ntiles=%d x K=%d codes exceed 2 GiB", fn, ntiles,
             K);
  a = WqArgs{c.X,        c.Q,    reinterpret_cast<const float*>(c.scale), c.Y,  c.ldx,    c.ldy,     M, K, N, ntiles, KK,
             c.residual, c.sout, c.gnext,                                 c.yg, c.rstats, c.rgroups, c.eps};
  return 0;
}

// The <= 16-row entries (fo_gemm_w8 / _w4 / _w6): k_wq_xs for the SwiGLU pair at K = 3584, k_wq_sk for long-K plain
// launches with a workspace, k_wq otherwise
template <typename F>
int wq_gemm(const WqEntry& en, const WqCall& c) {
  // every check before the first HIP call
  WqArgs a;
  int units;
  if (const int rc = wq_args<F>(en, c, a, units)) return rc;
  const int KK = a.KK;
  hipStream_t stream = c.stream;
  if (c.sgroups) *c.sgroups = units;
  if (c.swiglu && c.K == 3584) {
    const int G = units < wq_cus() ? units : wq_cus();
    // F::XS; F::XS_ENV = F::XS_ALT_ARG runs F::XS_ALT (A/B only)
    static const bool alt = [] { const char* e = getenv(F::XS_ENV); return e && atoi(e) == F::XS_ALT_ARG; }();
    if (alt)
      hipLaunchKernelGGL((k_wq_xs<F, F::XS_ALT.nw, F::XS_ALT.kpw>), dim3(G), dim3(F::XS_ALT.nw * 64), 0, stream, a, units);
    else hipLaunchKernelGGL((k_wq_xs<F, F::XS.nw, F::XS.kpw>), dim3(G), dim3(F::XS.nw * 64), 0, stream, a, units);
    F::count(WQ_XS);
    return wq_check(en.fn, " (xs)");
  }
  // long-K plain projections (K > 8 Ki - F::COLS; the Qwen2 down: 224 tiles x 18944 columns): 4 tiles per workgroup, K
  // split over the workgroups until the grid is about one workgroup per CU, merged in the launch (needs the caller's
  // workspace and zeroed tickets; without them the one-tile form below serves)
  if (!c.swiglu && KK >= 8192 / F::COLS && units >= 16 && c.ws && c.counters) {
    constexpr int NT = 4, NW = 8;
    const int groups = (units + NT - 1) / NT;
    int S = wq_cus() / groups;
    S = S < 1 ? 1 : (S > 8 ? 8 : S);
    if (S == 1 || ((long long)S * 16 * groups * NT * 16 <= c.ws_floats && groups <= (1 << 20))) {
      hipLaunchKernelGGL((k_wq_sk<F, NW, NT>), dim3(groups, S), dim3(NW * 64), 0, stream, a, S, c.ws, c.counters);
      F::count(WQ_SK);
      return wq_check(en.fn, " (split K)");
    }
  }
  const bool wide = KK >= 2048 / F::COLS;   // 16 waves where each still gets code steps to keep in flight
  if (c.swiglu) {
    if (wide) hipLaunchKernelGGL((k_wq<F, 16, true>), dim3(units), dim3(1024), 0, stream, a);
    else hipLaunchKernelGGL((k_wq<F, 4, true>), dim3(units), dim3(256), 0, stream, a);
  } else {
    if (wide) hipLaunchKernelGGL((k_wq<F, 16, false>), dim3(units), dim3(1024), 0, stream, a);
    else hipLaunchKernelGGL((k_wq<F, 4, false>), dim3(units), dim3(256), 0, stream, a);
  }
  F::count(WQ_GENERAL);
  return wq_check(en.fn);
}

// The lm_head entries (fo_gemm_w*_head): k_wq_xs's plain form, compiled for K = 3584
template <typename F>
int wq_head(const WqEntry& en, const float* X, int ldx, int M, int K, const void* Q, const void* scale, int ntiles,
            int N, float* Y, int ldy, hipStream_t stream) {
  // every check before the first HIP call
  WqArgs a;
  int tiles;
  const WqCall c{X,       ldx, M,       K,       Q,   scale,   ntiles,  N,       0,     Y, ldy, 0, nullptr, 0,
                 nullptr, nullptr, 0, 0.f, nullptr, nullptr, nullptr, nullptr, stream};
  if (const int rc = wq_args<F>(en, c, a, tiles)) return rc;
  FO_REQUIRE(K == 3584, "%s: K=%d, the X-stationary plain form is compiled for K = 3584 (%s serves any other K)", en.fn,
             K, F::GEMM);
  // units of two adjacent plain tiles dealt evenly to at most one workgroup per CU; the SwiGLU form's wave shape
  const int units = (ntiles + 1) / 2;
  const int G = units < wq_cus() ? units : wq_cus();
  hipLaunchKernelGGL((k_wq_xs<F, F::XS.nw, F::XS.kpw, false>), dim3(G), dim3(F::XS.nw * 64), 0, stream, a, units);
  F::count(WQ_HEAD);
  return wq_check(en.fn);
}

// The 17..64-row entries (fo_gemm_w*_rows).  NW waves x KPW code steps of X per K slice (hi in VGPRs, lo in LDS):
// F::ROWS[RB - 2][swiglu].  S slices of `per` code steps, units of two packed tiles, about one workgroup per CU.
// S > 1: the slabs are merged by a second launch (k_wq_rows_merge), one small workgroup per (tile, row block).
template <typename F, int RB, bool SW>
void wq_launch_rows(const WqArgs& a, int G, int S, int per, float* ws, hipStream_t stream) {
  constexpr WqShape sh = F::ROWS[RB - 2][SW];
  hipLaunchKernelGGL((k_wq_rows<F, sh.nw, sh.kpw, RB, SW>), dim3(G, S), dim3(sh.nw * 64), 0, stream, a, S, per, ws);
}
template <typename F>
int wq_rows(const WqEntry& en, const WqCall& c) {
  // every check before the first HIP call
  WqArgs a;
  int units;
  if (const int rc = wq_args<F>(en, c, a, units)) return rc;
  const int RB = (c.M + 15) / 16, sw = c.swiglu ? 1 : 0;
  const WqShape sh = F::ROWS[RB - 2][sw];
  const int S = (a.KK + sh.nw * sh.kpw - 1) / (sh.nw * sh.kpw), per = (a.KK + S - 1) / S;
  if (S > 1) {
    const long long need = (long long)S * RB * 16 * c.ntiles * 16;
    FO_REQUIRE(c.ws && need <= c.ws_floats,
               "%s: K=%d splits over %d workgroups: split-K workspace too small (%lld floats needed, %lld given)", en.fn,
               c.K, S, need, c.ws ? c.ws_floats : 0ll);
  }
  const int pairs = (c.ntiles + 1) / 2;
  const int per_split = wq_cus() / S < 1 ? 1 : wq_cus() / S;
  const int G = pairs < per_split ? pairs : per_split;
  if (c.sgroups) *c.sgroups = units;
  switch (2 * RB + sw) {
    case 4: wq_launch_rows<F, 2, false>(a, G, S, per, c.ws, c.stream); break;
    case 5: wq_launch_rows<F, 2, true>(a, G, S, per, c.ws, c.stream); break;
    case 6: wq_launch_rows<F, 3, false>(a, G, S, per, c.ws, c.stream); break;
    case 7: wq_launch_rows<F, 3, true>(a, G, S, per, c.ws, c.stream); break;
    case 8: wq_launch_rows<F, 4, false>(a, G, S, per, c.ws, c.stream); break;
    default: wq_launch_rows<F, 4, true>(a, G, S, per, c.ws, c.stream); break;
  }
  if (S > 1) {
    if (const int rc = wq_check(en.fn)) return rc;
    launch_merge<F::SCALED>(a, c.swiglu, units, RB, S, c.ws, c.stream);
  }
  F::count(WQ_ROWS);
  return wq_check(en.fn);
}

// What the two quantised q|k|v entries check beside wq_args (all on the host, before any HIP call), then
// QkvRopeArgs.  `fn` is the entry's name.
inline int qkv_rope_args(const char* fn, int N, const float* bias, const int* pos, const int* slot, const float* cos_t,
                         const float* sin_t, float* q_out, void* kc, void* vc, int H, int KVH, int hd, int PS,
                         int kv_bytes, QkvRopeArgs& r) {
  FO_REQUIRE(pos && slot && cos_t && sin_t && q_out && kc && vc,
             "%s: NULL pos, slot, cos_t, sin_t, q_out, kc or vc", fn);
  FO_REQUIRE(kv_bytes == 4 || kv_bytes == 2, "%s: kv_bytes %d (4 = fp32, 2 = bf16)", fn, kv_bytes);
  FO_REQUIRE(PS > 0, "%s: PS=%d (slots per page)", fn, PS);
  FO_REQUIRE(hd > 0 && (hd & 31) == 0, "%s: hd=%d must be a multiple of 32 (a tile pair holds columns i, i + hd/2)", fn,
             hd);
  FO_REQUIRE(H > 0 && KVH > 0 && (long long)N == ((long long)H + 2ll * KVH) * hd, "%s: N=%d != (H + 2 KVH) * hd (H=%d "
             "KVH=%d hd=%d)", fn, N, H, KVH, hd);
  r = QkvRopeArgs{bias, pos, slot, cos_t, sin_t, q_out, kc, vc, H, KVH, hd, PS, kv_bytes == 2 ? 1 : 0,
                  fo::kv_bf16_values()};
  return 0;
}

// The fused q|k|v entries (fo_gemm_w8_qkv_rope / fo_gemm_w4_qkv_rope): one workgroup per rope tile pair (Qwen2-7B:
// 144); 16 waves where each still gets code steps to keep in flight
template <typename F>
int wq_qkv_rope(const WqEntry& en, const float* X, int ldx, int M, int K, const void* Q, const void* scale, int ntiles,
                int N, const float* bias, const float* rstats, int rgroups, float eps, const int* pos, const int* slot,
                const float* cos_t, const float* sin_t, float* q_out, void* kc, void* vc, int H, int KVH, int hd, int PS,
                int kv_bytes, hipStream_t stream) {
  // every check before the first HIP call (q_out stands where wq_args expects an output: N floats per row)
  WqArgs a;
  QkvRopeArgs r;
  int tiles;
  const WqCall c{X,       ldx,    M,       K,   Q,       scale,   ntiles,  N,       0,     q_out, N, 0, nullptr, 0,
                 nullptr, rstats, rgroups, eps, nullptr, nullptr, nullptr, nullptr, stream};
  if (const int rc = wq_args<F>(en, c, a, tiles)) return rc;
  if (const int rc = qkv_rope_args(en.fn, N, bias, pos, slot, cos_t, sin_t, q_out, kc, vc, H, KVH, hd, PS, kv_bytes, r))
    return rc;
  const int pairs = ntiles / 2;
  if (a.KK >= 2048 / F::COLS) hipLaunchKernelGGL((k_wq_qkv<F, 16>), dim3(pairs), dim3(1024), 0, stream, a, r);
  else hipLaunchKernelGGL((k_wq_qkv<F, 4>), dim3(pairs), dim3(256), 0, stream, a, r);
  F::count(WQ_QKV);
  return wq_check(en.fn);
}

}  // namespace
