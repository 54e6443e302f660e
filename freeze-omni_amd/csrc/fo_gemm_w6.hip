// Weight-only MXFP6 (OCP e2m3 codes, one power-of-two scale per 32 elements) GEMMs for the Qwen2 MLP at <= 16 rows
// (fo_gemm_w6; fo_gemm_w6_head for the lm_head: k_wq_xs's plain form) and at 17..64 rows (fo_gemm_w6_rows: k_wq_rows,
// then k_wq_rows_merge where K is split), and their quantiser.  This file holds what is MXFP6's own -- the decode, the
// streaming inner loop with its transpose, the format description Mxfp6 and the quantiser; the kernels and the host
// path are fo_gemm_wq.h's, instantiated on Mxfp6.
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
#include <atomic>

#include "fo_gemm_wq.h"

namespace {

typedef __attribute__((ext_vector_type(3))) unsigned u32x3;
typedef __attribute__((ext_vector_type(6))) unsigned u32x6;
typedef __attribute__((ext_vector_type(32))) __bf16 bf16x32;

// One lane's image of a code step: its two planes (codes 0..15, 16..31) and its row's scale dword as loaded (the
// lane's byte, lane >> 4, is taken where the image is decoded, so the load stays in flight until then)
struct W6Code {
  u32x3 p0, p1;
  unsigned s;
};
struct W6Frag {
  bf16x8 f[4];    // the B fragments of the four MFMA sub-steps
};

// 32 e2m3 codes times 2^(sb - 127) -> 32 bf16, one instruction
__device__ __forceinline__ W6Frag dec6(const W6Code& q, unsigned sb) {
  const u32x6 v = {q.p0[0], q.p0[1], q.p0[2], q.p1[0], q.p1[1], q.p1[2]};
  const bf16x32 w = __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(v, __uint_as_float(sb << 23));
  return __builtin_bit_cast(W6Frag, w);
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

// The format description (fo_gemm_wq.h): 128-column code steps of four fragments, 1.5 KiB a tile, no column scale
struct Mxfp6 {
  static constexpr int COLS = 128, FR = 4, STEP = 1536;
  static constexpr bool SCALED = false;
  typedef W6Code Code;
  typedef WqMxSrd Srd;
  static __device__ __forceinline__ Code zero() { return W6Code{u32x3{0u, 0u, 0u}, u32x3{0u, 0u, 0u}, 0u}; }
  static __device__ __forceinline__ Srd srd(const WqArgs& a) { return wq_mx_srd<STEP>(a); }
  static __device__ __forceinline__ Code load(const Srd& d, int lane, int step) {   // step = tile * KK + code step
    W6Code q;
    q.p0 = __builtin_bit_cast(u32x3, __builtin_amdgcn_raw_buffer_load_b96(d.q, lane * 12, step * STEP, 2));
    q.p1 = __builtin_bit_cast(u32x3, __builtin_amdgcn_raw_buffer_load_b96(d.q, 768 + lane * 12, step * STEP, 2));
    q.s = wq_mx_scale(d, lane, step);
    return q;
  }
  static __device__ __forceinline__ void decode(const Code& q, int lane, bf16x8 (&w)[FR]) {
    const W6Frag f = dec6(q, (q.s >> (8 * (lane >> 4))) & 0xffu);
#pragma unroll
    for (int h = 0; h < FR; ++h) w[h] = f.f[h];
  }
  // fragment j = sub-step j & 3 of the wave's code step j >> 2, lane group g the step's block of 32 columns from 32 g:
  // the layout's own assignment (a condition per lane group where K % 128 != 0)
  static __device__ __forceinline__ int xcol(int g, int j) { return 32 * g + 128 * (j >> 2) + 8 * (j & 3); }
  static __device__ __forceinline__ int xblock(int g, int j) { return 32 * g + 128 * (j >> 2); }
  template <int NT, int U>
  static __device__ __forceinline__ void accumulate(const WqArgs& a, const Srd& d, const float* xp, int lane, int tile0,
                                                    int kb, int ke, f32x4 (&acc)[NT]);
  static constexpr int U_PAIR = 1, U_PLAIN = 1, U_SK = 1;   // code steps in flight
  // xs: 14 waves x 2 code steps; FO_W6_XS=7 runs 7 x 4 (A/B only)
  static constexpr WqShape XS = {14, 2}, XS_ALT = {7, 4};
  static constexpr const char* XS_ENV = "FO_W6_XS";
  static constexpr int XS_ALT_ARG = 7;
  // (the lo fragments are re-read from LDS per tile, as they always were here: 112 VGPRs against 122 hoisted, which
  // no longer spills now that the wave index is a scalar, but timed 67.5 against 67.0 us on the head at 1 row with a
  // spread of 0.3: profiles/gemm_wq_fold_ab.txt)
  static constexpr bool XS_REREAD_LO = true;
  // rows: Mxfp4's shapes at 3 and 4 row blocks (7 x 1 for SwiGLU, 8 x 1 / 6 x 1 for plain).  At 2 row blocks its 7 x 2
  // does not fit here: the two-deep code buffer is 2 x 2 x KPW x 7 dwords a lane against MXFP4's x 5, and both 7 x 2
  // instantiations spilled (256 VGPRs, 8 and 16 bytes of scratch a lane), so 2 row blocks run 7 x 1 (DESIGN 5.10 has
  // every instantiation's figures)
  static constexpr WqShape ROWS[3][2] = {{{7, 1}, {7, 1}}, {{8, 1}, {7, 1}}, {{6, 1}, {7, 1}}};
  static constexpr const char* GEMM = "fo_gemm_w6";
  static constexpr const char* QUANT = "the E8M0 block bytes of fo_quant_w6";
  static constexpr bool PAIR_CHECK = true;
  static void count(WqForm f);
};

// acc[t] = X[rows 0..16, code steps [kb, ke)] . (packed tile tile0 + t)^T for t < NT: U code steps in flight, each X
// fragment loaded and split once for the NT tiles.  xp: the lane's row at column 8 (lane >> 4).  X is loaded as the
// bf16 and MXFP4 kernels load it -- load j of lane (r, g') reads columns 128 kk + 32 j + 8 g' .. + 7, so the four lane
// groups of a row share one 128-byte line (the layout's own assignment, 32 consecutive columns per lane, touches four
// times as many lines per load and cost the down projection 5 us at 16 rows) -- and the split fragments are transposed
// across the lane groups (xpose4) into the layout's assignment: lane (r, g) sub-step t = columns 128 kk + 32 g + 8 t.
// A 32-column block at or past K (K % 128 != 0: load j of the last code step, wave-uniform) reads no X and holds
// zeros, which the transpose hands to lane group j as its zero A fragments; the other groups of the same MFMAs are live.
template <int NT, int U>
__device__ __forceinline__ void Mxfp6::accumulate(const WqArgs& a, const Srd& d, const float* xp, int lane, int tile0,
                                                  int kb, int ke, f32x4 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = kb; k0 < ke; k0 += U) {
    Code q[U][NT];
    float4 x[U][8];
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int kk = k0 + i;
      if (kk < ke) {
#pragma unroll
        for (int t = 0; t < NT; ++t) q[i][t] = load(d, lane, (tile0 + t) * a.KK + kk);
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
          bf16x8 w[FR];
          decode(q[i][t], lane, w);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi[j], w[j], acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo[j], w[j], acc[t], 0, 0, 0);
          }
        }
      }
    }
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

// the launch counters (fo_gemm_w6_counts): fo_gemm_w6's general, xs and sk forms, and fo_gemm_w6_head; and the calls of
// fo_gemm_w6_rows (fo_gemm_w6_rows_count)
std::atomic<long long> g_w6_launches[4];
std::atomic<long long> g_w6_rows_calls;
void Mxfp6::count(WqForm f) {
  if (f == WQ_ROWS) g_w6_rows_calls.fetch_add(1, std::memory_order_relaxed);
  else g_w6_launches[f].fetch_add(1, std::memory_order_relaxed);   // (WQ_GENERAL, WQ_XS, WQ_SK, WQ_HEAD: slots 0..3)
}

// the entries: name, row band, what the refusal says of the band
constexpr WqEntry E_GEMM = {"fo_gemm_w6", 1, 16, "the MXFP6 stream serves M <= 16 (more rows run the bf16 image)"};
constexpr WqEntry E_HEAD = {"fo_gemm_w6_head", 1, 16, E_GEMM.serves};
constexpr WqEntry E_ROWS = {"fo_gemm_w6_rows", 17, 64,
                            "this MXFP6 stream serves 17 <= M <= 64 (fo_gemm_w6 serves M <= 16, more than 64 rows run "
                            "the bf16 image)"};

}  // namespace

extern "C" {

long long fo_quant_w6_bytes(int N, int K) { return (long long)((N + 15) / 16) * ((K + 127) / 128) * Mxfp6::STEP; }
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
  return wq_gemm<Mxfp6>(E_GEMM, FO_WQ_CALL);
}

int fo_gemm_w6_head(const float* X, int ldx, int M, int K, const void* Q, const void* scale, int ntiles, int N,
                    float* Y, int ldy, hipStream_t stream) {
  return wq_head<Mxfp6>(E_HEAD, X, ldx, M, K, Q, scale, ntiles, N, Y, ldy, stream);
}

int fo_gemm_w6_rows(const float* X, int ldx, int M, int K, const void* Q, const void* scale, int ntiles, int N,
                    int swiglu, float* Y, int ldy, int residual, float* ws, long long ws_floats, int* counters,
                    const float* rstats, int rgroups, float eps, float* sout, const float* gnext, float* yg,
                    int* sgroups, hipStream_t stream) {
  return wq_rows<Mxfp6>(E_ROWS, FO_WQ_CALL);
}

}  // extern "C"
