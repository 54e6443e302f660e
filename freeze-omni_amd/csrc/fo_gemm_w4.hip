// Weight-only MXFP4 (OCP e2m1 codes, one power-of-two scale per 32 elements) GEMMs for the Qwen2 MLP at <= 16 rows
// (fo_gemm_w4; fo_gemm_w4_head for the lm_head: k_w4_xs's plain form) and at 17..64 rows (fo_gemm_w4_rows), and their
// quantiser.
//
//   W'[n, k] = q[n, k] * 2^e[n, k / 32]   q an e2m1 code (0, 0.5, 1, 1.5, 2, 3, 4, 6 and a sign bit), e one integer
//                                         per (output row, block of 32 columns), stored as the E8M0 byte e + 127
//   Y[M, N]  = epilogue( X[M, K] (fp32, split into bf16 hi + lo) . W'^T )
//
// An e2m1 value has 2 significant bits, so q * 2^e is exactly a bf16 value: W' has an exact bf16 image, which the
// engine keeps packed for the bf16 kernels and runs wherever the codes are not streamed.  The kernels here stream the codes -- a quarter of
// the bytes of that image, plus 1/32 of scales -- decode them to bf16 in registers with the block scale applied
// (v_cvt_scalef32_pk_bf16_fp4: exact) and run the same bf16 MFMAs, so both paths compute X . W'^T to the
// accumulation-order difference that already exists between the bf16 kernels.  The block scale cannot multiply the
// sum as the FP8 stream's column scale does; the epilogue (fo_gemm_wq.h) runs without one.  Results are deterministic
// in every form.
//
// Code layout (include/fo_hip.h): [tile][K128][64 lanes][16 bytes], a lane's dword j being its 8-element MFMA
// B fragment of k-step 4 s + j (two codes per byte, the lower column in the low nibble), K padded to a multiple of
// 128 with zero codes; scale bytes [tile][K128][16 rows][4].  This file holds what is MXFP4's own -- the decode, the
// streaming inner loop, the format description Mxfp4 and the quantiser; the kernels and the host path are
// fo_gemm_wq.h's, instantiated on Mxfp4.  fo_gemm_w4: k_wq (general), k_wq_xs (the SwiGLU pair at K = 3584) or k_wq_sk
// (long-K plain); fo_gemm_w4_head: k_wq_xs's plain form; fo_gemm_w4_qkv_rope: k_wq_qkv; fo_gemm_w4_rows: k_wq_rows, then
// k_wq_rows_merge where K is split.
#include <atomic>

#include "fo_gemm_wq.h"

namespace {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// 8 e2m1 codes (one dword) times 2^(sb - 127) -> 8 bf16: one convert per byte (the low nibble is the lower column)
__device__ __forceinline__ bf16x8 dec4(unsigned d, unsigned sb) {
  const float s = __uint_as_float(sb << 23);
  u32x4 r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 0));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 1));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 2));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 3));
  return __builtin_bit_cast(bf16x8, r);
}

// One lane's image of a code step: its four fragment dwords and its row's four scale bytes (byte j: k-step j)
struct W4Code {
  u32x4 c;
  unsigned s;
};
__device__ __forceinline__ W4Code w4_load(const WqMxSrd& d, int lane, int step) {   // step = tile * KK + code step
  return W4Code{__builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(d.q, lane * 16, step * 1024, 2)),
                wq_mx_scale(d, lane, step)};
}

// The format description (fo_gemm_wq.h): 128-column code steps of four fragments, 1 KiB a tile, no column scale
struct Mxfp4 {
  static constexpr int COLS = 128, FR = 4, STEP = 1024;
  static constexpr bool SCALED = false;
  typedef W4Code Code;
  typedef WqMxSrd Srd;
  static __device__ __forceinline__ Code zero() { return W4Code{u32x4{0u, 0u, 0u, 0u}, 0u}; }
  static __device__ __forceinline__ Srd srd(const WqArgs& a) { return wq_mx_srd<STEP>(a); }
  static __device__ __forceinline__ Code load(const Srd& d, int lane, int step) { return w4_load(d, lane, step); }
  static __device__ __forceinline__ void decode(const Code& q, int, bf16x8 (&w)[FR]) {
#pragma unroll
    for (int h = 0; h < FR; ++h) w[h] = dec4(q.c[h], (q.s >> (8 * h)) & 0xffu);
  }
  // fragment j = k-step j of the wave's code steps, lane group g its columns 8 g .. + 7
  static __device__ __forceinline__ int xcol(int g, int j) { return 8 * g + 32 * j; }
  static __device__ __forceinline__ int xblock(int, int j) { return 32 * j; }
  template <int NT, int U>
  static __device__ __forceinline__ void accumulate(const WqArgs& a, const Srd& d, const float* xp, int lane, int tile0,
                                                    int kb, int ke, f32x4 (&acc)[NT]);
  // code steps in flight (32 X floats per code step: Fp8's register budget at half the steps); the split-K form one
  // (two measured 18.6 / 19.5 / 21.8 us at 1 / 8 / 16 rows against 18.0 / 19.5 / 20.9 for one)
  static constexpr int U_PAIR = 1, U_PLAIN = 2, U_SK = 1;
  // xs: 14 waves x 2 code steps (21.0 / 23.5 us at 8 / 16 rows against 21.6 / 24.3 for 7 x 4, which FO_W4_XS=7 runs:
  // A/B only)
  static constexpr WqShape XS = {14, 2}, XS_ALT = {7, 4};
  static constexpr const char* XS_ENV = "FO_W4_XS";
  static constexpr int XS_ALT_ARG = 7;
  // (the lo fragments stay hoisted in registers, as they always were here; re-reading them per tile fits as well -- 94
  // against 106 VGPRs -- and timed level: profiles/gemm_wq_fold_ab.txt)
  static constexpr bool XS_REREAD_LO = false;
  // rows: starting from Fp8's columns per wave (7 x 2 at 2 row blocks, 7 x 1 at 3, 6 x 1 at 4) and keeping what measured
  // best per GEMM against one alternative each (builder-run, profiles/mlp_mxfp4_rows_gemm_ab.txt; gate/up / down in
  // us): 2 row blocks 7 x 2 (41.6 / 26.4 against 42.2 / 27.8 for 7 x 1); 3 row blocks 7 x 1 for SwiGLU (54.2 against
  // 55.1 for 8 x 1) and 8 x 1 for plain (32.5 against 35.6 for 7 x 1); 4 row blocks 7 x 1 for SwiGLU, which reduces a
  // tile at a time (70.9 against 73.3 for 6 x 1), and 6 x 1 for plain (45.1 against 46.3)
  static constexpr WqShape ROWS[3][2] = {{{7, 2}, {7, 2}}, {{8, 1}, {7, 1}}, {{6, 1}, {7, 1}}};
  static constexpr const char* GEMM = "fo_gemm_w4";
  static constexpr const char* QUANT = "the E8M0 block bytes of fo_quant_w4";
  static constexpr bool PAIR_CHECK = true;
  static void count(WqForm f);
};

// acc[t] = X[rows 0..16, code steps [kb, ke)] . (packed tile tile0 + t)^T for t < NT: U code steps in flight, each X
// fragment loaded and split once for the NT tiles.  A k-step at or past K (K % 128 != 0: zero codes) reads no X and
// runs no MFMA.
template <int NT, int U>
__device__ __forceinline__ void Mxfp4::accumulate(const WqArgs& a, const Srd& d, const float* xp, int lane,
                                                    int tile0, int kb, int ke, f32x4 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = kb; k0 < ke; k0 += U) {
    W4Code q[U][NT];
    float4 x[U][8];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int kk = k0 + i;
      if (kk < ke) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
          q[i][t] = w4_load(d, lane, (tile0 + t) * a.KK + kk);

        const float* p = xp + (size_t)kk * 128;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (kk * 128 + 32 * j < a.K) {
            x[i][2 * j] = reinterpret_cast<const float4*>(p + 32 * j)[0];
            x[i][2 * j + 1] = reinterpret_cast<const float4*>(p + 32 * j)[1];
          }
      }
    }
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int kk = k0 + i;
      if (kk < ke) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (kk * 128 + 32 * j < a.K) {
            bf16x8 hi, lo;
            split8(x[i][2 * j], x[i][2 * j + 1], hi, lo);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
              const bf16x8 w = dec4(q[i][t].c[j], (q[i][t].s >> (8 * j)) & 0xffu);
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, w, acc[t], 0, 0, 0);
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, w, acc[t], 0, 0, 0);
            }
          }
      }
    }
  }
}

// ---- quantiser.  One workgroup per source row n, one 32-column block per thread and pass: the block's amax, e from
// its exponent and mantissa (the smallest integer with amax * 2^-e <= 6 = 1.5 * 2^2, at least -125 so that every
// non-zero q * 2^e is a normal bf16; 0 for an all-zero block), W * 2^-e (exact, or an underflow that rounds to 0 anyway)
// rounded to the nearest e2m1 magnitude, ties to the even code, the sign bit copied; then the block's four dwords to
// their fragment positions (lane group g = columns 8 g .. + 8 of the k-step), its scale byte, and the 32 dequantised
// bf16 values to wdq.  Columns K .. 128 KK and rows N .. 16 ceil(N / 16) get zero codes and scale byte 127.
__device__ __forceinline__ unsigned e2m1_code(float v) {
  const float m = fabsf(v);
  const unsigned c = (unsigned)(m > 0.25f) + (unsigned)(m >= 0.75f) + (unsigned)(m > 1.25f) + (unsigned)(m >= 1.75f) +
                     (unsigned)(m > 2.5f) + (unsigned)(m >= 3.5f) + (unsigned)(m > 5.f);
  return c | ((__float_as_uint(v) >> 28) & 8u);
}

__global__ __launch_bounds__(256) void k_quant_w4(const void* W, int src_bf16, int N, int K, int ldw, unsigned char* q,
                                                  unsigned char* scale, bf16_t* wdq, int KK, int tile_base,
                                                  int tile_stride) {
  const int n = blockIdx.x;
  auto at = [&](int k) {
    return src_bf16 ? bf2f(reinterpret_cast<const bf16_t*>(W)[(size_t)n * ldw + k])
                    : reinterpret_cast<const float*>(W)[(size_t)n * ldw + k];
  };
  const size_t dt = (size_t)tile_base + (size_t)(n >> 4) * tile_stride;
  for (int b = threadIdx.x; b < KK * 4; b += 256) {   // block b: columns 32 b .. + 32, k-step b & 3 of code step b >> 2
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
      e = (int)(bits >> 23) - 127 - 2 + ((bits & 0x7fffffu) > 0x400000u ? 1 : 0);
      e = max(e, -125);
    }
    const float s = __uint_as_float((unsigned)(e + 127) << 23), inv = __uint_as_float((unsigned)(127 - e) << 23);
    const int kk = b >> 2, ks = b & 3;
    scale[((dt * KK + kk) * 16 + (n & 15)) * 4 + ks] = (unsigned char)(e + 127);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      unsigned dw = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned c = e2m1_code(v[8 * g + j] * inv);
        dw |= c << (4 * j);
        if (wdq && live) {
          const float mag = (c & 7u) < 4u ? 0.5f * (float)(c & 7u) : (float)(((c & 1u) + 2u) << (((c & 7u) >> 1) - 2u));
          wdq[(size_t)n * K + 32 * b + 8 * g + j] = f2bf(__uint_as_float(__float_as_uint(mag * s) | ((c & 8u) << 28)));
        }
      }
      *reinterpret_cast<unsigned*>(q + ((dt * KK + kk) * 64 + 16 * g + (n & 15)) * 16 + 4 * ks) = dw;
    }
  }
}

// the launch counters of the three <= 16-row forms (fo_gemm_w4_counts): general, xs, sk; and the calls of
// fo_gemm_w4_rows (fo_gemm_w4_rows_count)
std::atomic<long long> g_w4_launches[3];
std::atomic<long long> g_w4_rows_calls;
void Mxfp4::count(WqForm f) {
  if (f == WQ_HEAD) fo::count_head(1);
  else if (f == WQ_QKV) fo::count_qkv_quant(1);
  else if (f == WQ_ROWS) g_w4_rows_calls.fetch_add(1, std::memory_order_relaxed);
  else g_w4_launches[f].fetch_add(1, std::memory_order_relaxed);   // (WQ_GENERAL, WQ_XS, WQ_SK: slots 0..2)
}

// the entries: name, row band, what the refusal says of the band
constexpr WqEntry E_GEMM = {"fo_gemm_w4", 1, 16, "the MXFP4 stream serves M <= 16 (more rows run the bf16 image)"};
constexpr WqEntry E_HEAD = {"fo_gemm_w4_head", 1, 16,
                            "the MXFP4 head stream serves M <= 16 (more rows run the bf16 image)"};
constexpr WqEntry E_QKV = {"fo_gemm_w4_qkv_rope", 1, 16,
                           "the MXFP4 q|k|v stream serves M <= 16 (more rows run the bf16 image)"};
constexpr WqEntry E_ROWS = {"fo_gemm_w4_rows", 17, 64,
                            "this MXFP4 stream serves 17 <= M <= 64 (fo_gemm_w4 serves M <= 16, more than 64 rows run "
                            "the bf16 image)"};

}  // namespace

extern "C" {

long long fo_quant_w4_bytes(int N, int K) { return (long long)((N + 15) / 16) * ((K + 127) / 128) * 1024; }
long long fo_quant_w4_scale_bytes(int N, int K) { return (long long)((N + 15) / 16) * ((K + 127) / 128) * 64; }

int fo_quant_w4(const void* W, int src_bf16, int N, int K, int ldw, void* q, void* scale, void* wdq, int tile_base,
                int tile_stride, hipStream_t stream) {
  FO_REQUIRE(W && q && scale, "fo_quant_w4: NULL W, q or scale");
  FO_REQUIRE(N > 0 && K > 0 && ldw >= K, "fo_quant_w4: bad shape N=%d K=%d ldw=%d", N, K, ldw);
  FO_REQUIRE((K & 31) == 0, "fo_quant_w4: K=%d must be a multiple of 32 (the scale block)", K);
  FO_REQUIRE(tile_base >= 0 && tile_stride >= 1, "fo_quant_w4: bad tile_base=%d tile_stride=%d", tile_base,
             tile_stride);
  const int nt = (N + 15) / 16;
  hipLaunchKernelGGL(k_quant_w4, dim3(nt * 16), dim3(256), 0, stream, W, src_bf16, N, K, ldw, (unsigned char*)q,
                     (unsigned char*)scale, (bf16_t*)wdq, (K + 127) / 128, tile_base, tile_stride);
  return fo::check_launch("fo_quant_w4");
}

int fo_gemm_w4_counts(long long* out, int n) {
  for (int i = 0; out && i < n && i < 3; ++i) out[i] = g_w4_launches[i].load(std::memory_order_relaxed);
  return 3;
}
int fo_gemm_w4_counts_reset(void) {
  for (int i = 0; i < 3; ++i) g_w4_launches[i].store(0, std::memory_order_relaxed);
  g_w4_rows_calls.store(0, std::memory_order_relaxed);
  return 0;
}
long long fo_gemm_w4_rows_count(void) { return g_w4_rows_calls.load(std::memory_order_relaxed); }

int fo_gemm_w4(const float* X, int ldx, int M, int K, const void* Q, const void* scale, int ntiles, int N, int swiglu,
               float* Y, int ldy, int residual, float* ws, long long ws_floats, int* counters, const float* rstats,
               int rgroups, float eps, float* sout, const float* gnext, float* yg, int* sgroups, hipStream_t stream) {
  return wq_gemm<Mxfp4>(E_GEMM, FO_WQ_CALL);
}

int fo_gemm_w4_head(const float* X, int ldx, int M, int K, const void* Q, const void* scale, int ntiles, int N,
                    float* Y, int ldy, hipStream_t stream) {
  return wq_head<Mxfp4>(E_HEAD, X, ldx, M, K, Q, scale, ntiles, N, Y, ldy, stream);
}

int fo_gemm_w4_qkv_rope(const float* X, int ldx, int M, int K, const void* Q, const void* scale, int ntiles, int N,
                        const float* bias, const float* rstats, int rgroups, float eps, const int* pos, const int* slot,
                        const float* cos_t, const float* sin_t, float* q_out, void* kc, void* vc, int H, int KVH, int hd,
                        int PS, int kv_bytes, hipStream_t stream) {
  return wq_qkv_rope<Mxfp4>(E_QKV, X, ldx, M, K, Q, scale, ntiles, N, bias, rstats, rgroups, eps, pos, slot, cos_t,
                            sin_t, q_out, kc, vc, H, KVH, hd, PS, kv_bytes, stream);
}

int fo_gemm_w4_rows(const float* X, int ldx, int M, int K, const void* Q, const void* scale, int ntiles, int N,
                    int swiglu, float* Y, int ldy, int residual, float* ws, long long ws_floats, int* counters,
                    const float* rstats, int rgroups, float eps, float* sout, const float* gnext, float* yg,
                    int* sgroups, hipStream_t stream) {
  return wq_rows<Mxfp4>(E_ROWS, FO_WQ_CALL);
}

}  // extern "C"
