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
// B-fragments of two consecutive 32-column k-steps, K padded to a multiple of 64 with zero codes.  This file holds what
// is e4m3's own -- the decode, the streaming inner loop, the format description Fp8, the 65..128-row kernel and the
// quantiser; the kernels and the host path of every other entry are fo_gemm_wq.h's, instantiated on Fp8:
//  * fo_gemm_w8, <= 16 rows: k_wq (general), k_wq_xs (the SwiGLU pair at K = 3584) or k_wq_sk (long-K plain);
//  * fo_gemm_w8_head, <= 16 rows: k_wq_xs's plain form at K = 3584 (the Qwen2 lm_head);
//  * fo_gemm_w8_qkv_rope, <= 16 rows: k_wq_qkv, k_wq's pair form with the fused q|k|v epilogue (bias, RoPE, paged-KV
//    append) over the rope-paired tile order of PackedLinear(rope_hd=...);
//  * fo_gemm_w8_rows, 17..64 rows: k_wq_rows, then k_wq_rows_merge where K is split;
//  * fo_gemm_w8_rows128, 65..128 rows: k_w8_rows128, then k_wq_rows_merge.
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

// The format description (fo_gemm_wq.h): 64-column code steps of two fragments, 1 KiB a tile, a column scale in the
// epilogue; a lane's image of a code step is its 16 bytes.
struct Fp8 {
  static constexpr int COLS = 64, FR = 2, STEP = 1024;
  static constexpr bool SCALED = true;
  typedef u32x4 Code;
  typedef __amdgpu_buffer_rsrc_t Srd;   // exactly the codes (ntiles * KK KiB): a tile at or past ntiles loads zero codes
  static __device__ __forceinline__ Code zero() { return u32x4{0u, 0u, 0u, 0u}; }
  static __device__ __forceinline__ Srd srd(const WqArgs& a) { return rsrc_of(a.Q, a.ntiles * a.KK * STEP); }
  static __device__ __forceinline__ Code load(const Srd& d, int lane, int step) {   // step = tile * KK + code step
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(d, lane * 16, step * STEP, 2));
  }
  static __device__ __forceinline__ void decode(const Code& q, int, bf16x8 (&w)[FR]) {
    w[0] = dec8(q[0], q[1]);
    w[1] = dec8(q[2], q[3]);
  }
  // fragment j = k-step j of the wave's code steps, lane group g its columns 8 g .. + 7
  static __device__ __forceinline__ int xcol(int g, int j) { return 8 * g + 32 * j; }
  static __device__ __forceinline__ int xblock(int, int j) { return 32 * j; }
  template <int NT, int U>
  static __device__ __forceinline__ void accumulate(const WqArgs& a, const Srd& d, const float* xp, int lane, int tile0,
                                                    int kb, int ke, f32x4 (&acc)[NT]);
  // code steps in flight: the pair forms 2, the plain general form 4 (4 pair steps spill at 16 waves' 128 VGPRs)
  static constexpr int U_PAIR = 2, U_PLAIN = 4, U_SK = 2;
  // xs: 14 waves x 4 code steps (25.4 / 28.5 us at 8 / 16 rows against 27.0 / 29.4 for 8 x 7, which FO_W8_XS=8 runs:
  // A/B only)
  static constexpr WqShape XS = {14, 4}, XS_ALT = {8, 7};
  static constexpr const char* XS_ENV = "FO_W8_XS";
  static constexpr int XS_ALT_ARG = 8;
  // (the lo fragments stay hoisted in registers, as they always were here.  Re-reading them per tile fits as well -- 106
  // against 112 VGPRs -- and timed level but for the gate/up at 16 rows in one of three scripts, 29.8 against 29.6 us
  // with a spread of 0.1: profiles/gemm_wq_fold_ab.txt)
  static constexpr bool XS_REREAD_LO = false;
  // rows: 7 x 4 at 2 row blocks, 7 x 2 at 3 and 6 x 2 at 4, the largest slices whose LDS still holds both tiles of a
  // unit in one reduction round (7 x 3 at 3 row blocks reduced a tile at a time and measured 63.8 against 58.1 us on
  // gate/up at 48 rows, 7 x 2 at 4 row blocks 48.7 against 46.7 us on the down at 64)
  static constexpr WqShape ROWS[3][2] = {{{7, 4}, {7, 4}}, {{7, 2}, {7, 2}}, {{6, 2}, {6, 2}}};
  static constexpr const char* GEMM = "fo_gemm_w8";
  static constexpr const char* QUANT = "the per-column 2^e of fo_quant_w8";
  static constexpr bool PAIR_CHECK = false;
  static void count(WqForm f) {
    if (f == WQ_HEAD) fo::count_head(0);
    else if (f == WQ_QKV) fo::count_qkv_quant(0);
    else fo::count_launch(f == WQ_XS ? FO_L_GEMM_W8_XS : (f == WQ_ROWS ? FO_L_GEMM_W8_ROWS : FO_L_GEMM_W8));
  }
};

// acc[t] = X[rows 0..16, code steps [kb, ke)] . (packed tile tile0 + t)^T for t < NT: U code steps in flight, each X
// fragment loaded and split once for the NT tiles.  The codes' descriptor covers exactly the codes (ntiles * KK KiB): a
// tile at or past ntiles is out of its range and loads zero codes.
template <int NT, int U>
__device__ __forceinline__ void Fp8::accumulate(const WqArgs& a, const Srd& srd, const float* xp, int lane,
                                                  int tile0, int kb, int ke, f32x4 (&acc)[NT]) {
  const int voff = lane * 16;
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
//    k_wq_rows_merge, the next launch, sums the slabs in slice order and runs the epilogue.
template <int N>
__device__ __forceinline__ void w8_wait_vm_barrier() {
  // this wave's DMA down to N outstanding and its LDS reads done, then the workgroup barrier, in one opaque statement
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"i"(N) : "memory");
}

template <int NTC, int D>
__global__ __launch_bounds__(512) void k_w8_rows128(WqArgs a, int S, int G, int tiles_per, float* ws) {
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

// the entries: name, row band, what the refusal says of the band
constexpr WqEntry E_GEMM = {"fo_gemm_w8", 1, 16, "the FP8 stream serves M <= 16 (more rows run the bf16 image)"};
constexpr WqEntry E_HEAD = {"fo_gemm_w8_head", 1, 16, "the FP8 head stream serves M <= 16 (more rows run the bf16 image)"};
constexpr WqEntry E_QKV = {"fo_gemm_w8_qkv_rope", 1, 16,
                           "the FP8 q|k|v stream serves M <= 16 (more rows run the bf16 image)"};
constexpr WqEntry E_ROWS = {"fo_gemm_w8_rows", 17, 64,
                            "this FP8 stream serves 17 <= M <= 64 (fo_gemm_w8 serves M <= 16, more than 64 rows run the "
                            "bf16 image)"};
constexpr WqEntry E_ROWS128 = {"fo_gemm_w8_rows128", 65, 128,
                               "this FP8 stream serves 65 <= M <= 128 (fo_gemm_w8 serves M <= 16, fo_gemm_w8_rows 17..64, "
                               "more than 128 rows run the bf16 image)"};

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
  return wq_gemm<Fp8>(E_GEMM, FO_WQ_CALL);
}

int fo_gemm_w8_head(const float* X, int ldx, int M, int K, const void* Q, const float* scale, int ntiles, int N,
                    float* Y, int ldy, hipStream_t stream) {
  return wq_head<Fp8>(E_HEAD, X, ldx, M, K, Q, scale, ntiles, N, Y, ldy, stream);
}

int fo_gemm_w8_qkv_rope(const float* X, int ldx, int M, int K, const void* Q, const float* scale, int ntiles, int N,
                        const float* bias, const float* rstats, int rgroups, float eps, const int* pos, const int* slot,
                        const float* cos_t, const float* sin_t, float* q_out, void* kc, void* vc, int H, int KVH, int hd,
                        int PS, int kv_bytes, hipStream_t stream) {
  return wq_qkv_rope<Fp8>(E_QKV, X, ldx, M, K, Q, scale, ntiles, N, bias, rstats, rgroups, eps, pos, slot, cos_t, sin_t,
                          q_out, kc, vc, H, KVH, hd, PS, kv_bytes, stream);
}

int fo_gemm_w8_rows(const float* X, int ldx, int M, int K, const void* Q, const float* scale, int ntiles, int N,
                    int swiglu, float* Y, int ldy, int residual, float* ws, long long ws_floats, int* counters,
                    const float* rstats, int rgroups, float eps, float* sout, const float* gnext, float* yg,
                    int* sgroups, hipStream_t stream) {
  return wq_rows<Fp8>(E_ROWS, FO_WQ_CALL);
}

int fo_gemm_w8_rows128(const float* X, int ldx, int M, int K, const void* Q, const float* scale, int ntiles, int N,
                       int swiglu, float* Y, int ldy, int residual, float* ws, long long ws_floats, int* counters,
                       const float* rstats, int rgroups, float eps, float* sout, const float* gnext, float* yg,
                       int* sgroups, hipStream_t stream) {
  WqArgs a;
  int units;
  if (const int rc = wq_args<Fp8>(E_ROWS128, FO_WQ_CALL, a, units)) return rc;
  const int KK = a.KK;
  // The plan of k_gemm_rows (fo_gemm.hip plan_rows).  A workgroup's X over its K slice (512 B per column at 128 rows)
  // passes through its CU beside its codes (16 B per tile and column), so the tiles per workgroup are as many as the
  // accumulators and the LDS ring allow and K is split until the grid is about one workgroup per CU: SwiGLU K thirds
  // of up to 15 (gate, up) pairs (the Qwen2 gate/up: 3 x 85 workgroups of 28 tiles), plain 14 or 16 tiles and up to
  // 16 slices (the Qwen2 down: 16 x 16 workgroups of 14 tiles x 18.5 code steps).  Never more slices than code steps.
  const int RB = (M + 15) / 16, cus = wq_cus();
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
