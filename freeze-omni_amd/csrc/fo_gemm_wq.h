// What the weight-stream GEMMs over quantised codes share (fo_gemm_w8.hip: e4m3 codes with a scale per output column;
// fo_gemm_w4.hip: MXFP4 codes whose block scale is applied in the decode): the argument block, the X split, the
// epilogue, the consumer's rstd, the accumulator hand-off through LDS and the merge of the row streams' split-K slabs.
#pragma once
#include "fo_common.h"

namespace fo {
// the launch counters of the lm_head streams (fo_gemm_head_counts, fo_gemm_w4.hip): slot 0 fo_gemm_w8_head, slot 1
// fo_gemm_w4_head.  Counters of their own: these kernels have no FoLaunchKind.
void count_head(int slot);
// the launch counters of the quantised q|k|v streams (fo_gemm_qkv_quant_counts, fo_gemm_w4.hip): slot 0
// fo_gemm_w8_qkv_rope, slot 1 fo_gemm_w4_qkv_rope
void count_qkv_quant(int slot);
}  // namespace fo

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

struct W8Args {
  const float* X;
  const void* Q;       // codes in packed order
  const float* scale;  // [ntiles][16], packed tile order (fo_gemm_w4: the E8M0 block-scale bytes, read by the decode)
  float* Y;
  int ldx, ldy;
  int M, K, N;         // N: logical output columns (after SwiGLU pairing)
  int ntiles;          // packed 16-column tiles in Q
  int KK;              // code steps per tile: ceil(K / 64) (fo_gemm_w4: ceil(K / 128))
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
// fo_gemm_qkv_rope_kv's GemmArgs carry in their r* fields (fo_gemm.hip), beside W8Args.
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
// fp32 sums of packed tiles 2P / 2P + 1.  In this order: the FP8 column scales (SCALED; the MXFP4 sums carry their
// block scales already), the consumer's rstd, the bias, rotate_half RoPE at pos[rr] for q and k heads, the store: q to
// q_out, K and V to the paged cache at slot[rr].  Rows >= M (computed from a clamped row) are never stored.
template <bool SCALED>
__device__ __forceinline__ void wq_rope_epilogue(const W8Args& a, const QkvRopeArgs& r, int P, int rr, int c, float x1,
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
// the unit's (gate, up) tiles (SW) or of its one tile.  The column scale first (SCALED; the MXFP4 sums carry their
// block scales already), then the consumer's rstd, SwiGLU, the residual and the store; a producer also writes
// yg = y * gamma_next and the row's sum of squares over the unit's 16 columns.  Rows >= M (computed from a clamped
// row) are neither stored nor summed.
template <bool SW, bool SCALED = true>
__device__ __forceinline__ void w8_epilogue(const W8Args& a, int u, int groups, int rr, int c, float x1, float x2,
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
__device__ __forceinline__ void w8_rstd(const W8Args& a, float* rstd_s, int wave, int lane, int r0 = 0, int n = 16) {
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
__device__ __forceinline__ void w8_store_tile(Tile& tile, const f32x4 acc, int lane, int r0 = 0) {
#pragma unroll
  for (int i = 0; i < 4; ++i) tile[r0 + 4 * (lane >> 4) + i][lane & 15] = acc[i];
}

// The merge of the row-stream kernels' slabs (k_w8_rows, k_w8_rows128, k_w4_rows): workgroup (u, rb) = output tile u
// (SW: the (gate, up) pair) x row block rb, thread 16 rr + c one element: every split's partial summed in split order
// (8 loads in flight; a missing split adds 0), then the epilogue (SCALED: with the FP8 column scale).
template <bool SW, bool SCALED>
__global__ __launch_bounds__(256) void k_w8_rows_merge(W8Args a, int S, const float* ws, int rows) {
  constexpr int T = SW ? 2 : 1;
  __shared__ float rstd_s[128];   // (indexed by the row: up to k_w8_rows128's 8 row blocks)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = blockIdx.x, rb = blockIdx.y;
  if (a.rstats) {
    w8_rstd<4>(a, rstd_s, wave, lane, rb * 16, 16);
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
  w8_epilogue<SW, SCALED>(a, u, gridDim.x, rr, c, x[0], x[T - 1], rstd_s);
}

// k_w8_rows_merge over the S slabs of RB row blocks in `ws`
template <bool SCALED>
void launch_merge(const W8Args& a, int swiglu, int units, int RB, int S, const float* ws, hipStream_t stream) {
  if (swiglu)
    hipLaunchKernelGGL((k_w8_rows_merge<true, SCALED>), dim3(units, RB), dim3(256), 0, stream, a, S, ws, RB * 16);
  else
    hipLaunchKernelGGL((k_w8_rows_merge<false, SCALED>), dim3(units, RB), dim3(256), 0, stream, a, S, ws, RB * 16);
}

// What the two quantised q|k|v entries check beside w8_args / w4_args (all on the host, before any HIP call), then
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

}  // namespace
