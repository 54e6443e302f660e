// Attention for the Freeze-Omni hot path.
//
// 1. Decoder attention over a paged KV cache (Qwen2 in AudioLLM, Llama layers of the AR speech
//    decoder).  Reference: transformers Qwen2Attention/LlamaAttention reached from
//    models/audioLLM.py:482 and models/decoder/decoder.py:294-312 (DynamicCache concat per layer).
//    Here the cache is a pool of fixed-size pages per layer, laid out [page][kv_head][slot][hd]
//    (fp32, or bf16 for the Qwen2 stack's opt-in llm_kv="bf16") so one head's keys in a page are
//    contiguous; sequences own block tables, so a shared system prompt is shared pages and growth
//    never copies.
//    Ragged batch: every token carries (sequence, absolute position); causal mode lets a query
//    see keys at positions <= its own, full mode (the reference's eager attention with
//    attention_mask=None / all-ones masks, decoder.py:140,175,302) sees the whole sequence.
//    Work items group a sequence's batch tokens (x the GQA group of query heads sharing one kv
//    head) so its keys are read once per kv head; split-KV over key ranges sized from each item's
//    own key count at run time, merged in the same launch by the last split to finish (or, without
//    a ticket buffer, static splits merged by a combine kernel).
// 2. Encoder rel-pos attention over a per-user ring buffer (models/encoder/attention.py:407-459):
//    scores = ((q+u).K^T + (q+v).P^T)/sqrt(dk), no mask, no rel_shift; P rows come from a
//    table of linear_pos(sinusoid(position)) precomputed at load for every position.
#include <atomic>
#include <type_traits>

#include "fo_common.h"

namespace {

// Element o of the paged cache `base`: kv16: f2bf(x) as a 2-byte element of a bf16 cache; else fp32, the
// bf16 value under rkvb (fo_set_kv_bf16, as the q|k|v epilogues do).  One kernel serves both layouts, so the value
// that is rounded is computed by the same instructions.
__device__ __forceinline__ void kv_put(void* base, size_t o, float x, int kv16, int rkvb) {
  if (kv16) reinterpret_cast<bf16_t*>(base)[o] = f2bf(x);
  else reinterpret_cast<float*>(base)[o] = rkvb ? bf2f(f2bf(x)) : x;
}
__global__ __launch_bounds__(256) void k_rope_kv_write(const float* qkv, int ldq, int T, int H, int KVH, int hd,
                                                       const int* pos, const int* slot, const float* cos_t,
                                                       const float* sin_t, float* q_out, void* kc, void* vc,
                                                       int PS, int kv16, int rkvb) {
  const int t = blockIdx.x;
  const int half = hd >> 1;
  const float* row = qkv + (size_t)t * ldq;
  const int p = pos[t];
  const float* cs = cos_t + (size_t)p * half;
  const float* sn = sin_t + (size_t)p * half;
  const int sl = slot[t];
  const int page = sl / PS, off = sl % PS;
  // q heads then k heads: rotate pairs (i, i + hd/2)
  for (int e = threadIdx.x; e < (H + KVH) * half; e += blockDim.x) {
    const int h = e / half, i = e % half;
    const float* src = row + (size_t)h * hd;  // q heads [0,H), k heads [H, H+KVH) are contiguous
    const float x1 = src[i], x2 = src[i + half];
    const float c = cs[i], s = sn[i];
    const float o1 = x1 * c - x2 * s;
    const float o2 = x2 * c + x1 * s;
    if (h < H) {
      q_out[(size_t)t * H * hd + (size_t)h * hd + i] = o1;
      q_out[(size_t)t * H * hd + (size_t)h * hd + i + half] = o2;
    } else {
      const size_t d = (((size_t)page * KVH + (h - H)) * PS + off) * hd;
      kv_put(kc, d + i, o1, kv16, rkvb);
      kv_put(kc, d + i + half, o2, kv16, rkvb);
    }
  }
  const float* vsrc = row + (size_t)(H + KVH) * hd;
  for (int e = threadIdx.x; e < KVH * hd; e += blockDim.x) {
    const int h = e / hd, i = e % hd;
    kv_put(vc, (((size_t)page * KVH + h) * PS + off) * hd + i, vsrc[e], kv16, rkvb);
  }
}

// The FP8 KV append: one wave per (token, kv head, K or V).  The q|k|v launch has written the token's K
// (after bias and RoPE) and V (after bias) as fp32 into a staging cache [kv head][stage row = token][hd]; the wave takes
// the row's maximum magnitude, the row exponent e of the weight quantiser (e4m3_row_exp), rounds x * 2^-e (exact) to
// e4m3fn by v_cvt_pk_fp8_f32 -- 4 elements a lane, one 4-byte store -- and stores the scale 2^e.  A non-finite element
// takes no part in the maximum and becomes the NaN code (sign | 0x7f), never a finite one.  Rows past T and lanes past
// hd / 4 load and store nothing.
__global__ __launch_bounds__(256) void k_kv8_append(const float* ksg, const float* vsg, int T, int KVH, int hd,
                                                    int srows, const int* slot, int PS, unsigned char* kc, float* ks,
                                                    unsigned char* vc, float* vs) {
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
  if (idx >= T * KVH * 2) return;
  const int isv = idx & 1, kvh = (idx >> 1) % KVH, t = (idx >> 1) / KVH;
  const bool on = 4 * lane < hd;
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  if (on) x = *reinterpret_cast<const float4*>((isv ? vsg : ksg) + ((size_t)kvh * srows + t) * hd + 4 * lane);
  auto mag = [](float v) { return fabsf(v) <= 3.4028234664e38f ? fabsf(v) : 0.f; };   // finite elements only
  const float amax = wave_max(fmaxf(fmaxf(mag(x.x), mag(x.y)), fmaxf(mag(x.z), mag(x.w))));
  const int e = e4m3_row_exp(amax);
  const float inv = pow2f(-e);
  int c = 0;
  c = __builtin_amdgcn_cvt_pk_fp8_f32(x.x * inv, x.y * inv, c, false);
  c = __builtin_amdgcn_cvt_pk_fp8_f32(x.z * inv, x.w * inv, c, true);
  unsigned u = (unsigned)c;
  auto nan_code = [&](float v, int sh) {
    if (!(fabsf(v) <= 3.4028234664e38f)) u = (u & ~(0xffu << sh)) | (((__float_as_uint(v) >> 24) & 0x80u) | 0x7fu) << sh;
  };
  nan_code(x.x, 0);
  nan_code(x.y, 8);
  nan_code(x.z, 16);
  nan_code(x.w, 24);
  const int sl = slot[t];
  const size_t row = ((size_t)(sl / PS) * KVH + kvh) * PS + sl % PS;
  if (on) *reinterpret_cast<unsigned*>((isv ? vc : kc) + row * hd + 4 * lane) = u;
  if (lane == 0) (isv ? vs : ks)[row] = pow2f(e);
}

#include "fo_attn_rows.h"

template <int HD, int NW = 4, int RT = 1, bool TR = false, int KVB = 4>
__global__ __launch_bounds__(NW * 64) void k_attn_mfma(AttnArgs a) {
  if constexpr (TR) {
#pragma nounroll
    for (int rep = 0; rep < (a.reps > 1 ? a.reps : 1); ++rep) {
      attn_rows_body<HD, NW, RT, TR>(a, blockIdx.x, blockIdx.y, blockIdx.z);
      __syncthreads();
    }
  } else {
    attn_rows_body<HD, NW, RT, TR, KVB>(a, blockIdx.x, blockIdx.y, blockIdx.z);
  }
}

// Single-row decode attention (the AR speech decoder's step, models/decoder/decoder.py:341-349: one
// token per session, one query head per kv head): one work group per (session, head) reads the
// session's keys once, in fp32 -- scores one key per thread (16-B loads of the key row), block
// max / sum, then P.V with the waves on interleaved keys, a float4 of the row per lane.  No MFMA tile would be
// more than 1/16 full here, and no split / merge round trip is needed at <= 4096 keys.
constexpr int DEC_MAXK = MAXPG * 16;
constexpr int DEC_NW = 8, DEC_NT = DEC_NW * 64;  // 8 waves: a key per thread up to 512 keys
// 4 bf16 of a bf16 cache, widened
__device__ __forceinline__ float4 bf4_to_f4(uint2 u) {
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
// 4 e4m3fn codes of an FP8 cache times their key's scale (a power of two), widened
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ float4 fp8x4_to_f4(unsigned w, float sc) {
  const f32x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, sc, false);
  const f32x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, sc, true);
  return make_float4(lo[0], lo[1], hi[0], hi[1]);
}
// The decode body's two sums, spelled out: 4 elements of a key's score, and a lane's 4 outputs += p * v.  Contraction
// is off, so the fmaf calls are the only fused operations and nothing is fused or regrouped around them -- every
// instantiation of the body (fp32 or bf16 cache, any kernel it is inlined into) then rounds at the same places.
__device__ __forceinline__ float dec_dot4(float s, const float* q, float4 k) {
#pragma clang fp contract(off)
  return s + fmaf(q[3], k.w, fmaf(q[2], k.z, fmaf(q[1], k.y, q[0] * k.x)));
}
__device__ __forceinline__ void dec_pv(float4& acc, float p, float4 v) {
#pragma clang fp contract(off)
  acc.x = fmaf(p, v.x, acc.x);
  acc.y = fmaf(p, v.y, acc.y);
  acc.z = fmaf(p, v.z, acc.z);
  acc.w = fmaf(p, v.w, acc.w);
}
// One (work item, head) of the decode attention; the normalised output row is left in o_s[HD] (LDS, visible to
// every thread after the call) and, unless to_lds_only, stored to out (+ the packed copy when armed).  Returns
// false when the host contract is broken (the row is then NaN, stored and in o_s).  h is the query head; its keys
// and values are those of kv head h / (H / KVH) (H == KVH for the AR decoder: the same head).
// KV16: a bf16 cache.  A key row is read as 16-byte loads of 8 bf16 and a lane's 4 elements of a V row as
// one 8-byte load, each widened to float; the sums are the fp32 form's own (dot4 / pv_add below, the same keys on the
// same lanes in the same order), so on a cache of bf16-representable values the two forms give the same result bit
// for bit.  dot4 / pv_add spell their multiply-adds out (dec_dot4 / dec_pv): left to the compiler, which products fuse
// with which adds depends on how each instantiation's loads vectorise, and the two forms then differ in the last bit.
// (16-byte V loads would halve the lanes per key and with them the key-to-lane interleave and the order of the
// cross-lane adds: not taken.)
// KVB 1: e4m3fn codes with one scale 2^e per (key, kv head) (a.ks / a.vs).  A key row is read as 16-byte
// loads of 16 codes and a lane's 4 elements of a V row as one 4-byte load; the scaled conversion
// (v_cvt_scalef32_pk_f32_fp8) widens them to the floats code * 2^e -- the widened elements of a bf16 cache holding those
// values -- and the sums are again dec_dot4 / dec_pv on the same lanes in the same order: the same result bit for bit.
template <int HD, int KVB = 4>
__device__ bool attn_decode_row(const AttnArgs& a, const int it, const int h, float* o_s, bool to_lds_only) {
  static_assert(HD % 4 == 0 && HD <= 128, "decode attention: head_dim");
  __shared__ float s_s[DEC_MAXK];
  __shared__ float q_s[HD];
  __shared__ float acc_s[DEC_NW][HD];
  __shared__ float red_s[DEC_NW];
  __shared__ int pg_s[MAXPG];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // items == NULL: the dense decode batch (item b = sequence b = token b), nothing to look up first
  const int seq = a.items ? a.items[3 * it] : it, t0 = a.items ? a.items[3 * it + 1] : it;
  // the visible-key count, the whole block-table row and q are requested together (none waits on
  // another); pages past the session's keys are staged but never dereferenced
  const int L = a.tok_nvis[t0];
  const int* bt = a.block_table + (size_t)seq * a.maxb;
  const int nb = a.maxb < MAXPG ? a.maxb : MAXPG;
  for (int i = tid; i < nb; i += DEC_NT) pg_s[i] = bt[i];
  const float* qr = a.q + ((size_t)t0 * a.H + h) * HD;
  for (int d = tid; d < HD; d += DEC_NT) q_s[d] = qr[d] * a.scale;
  float* orow = a.out + ((size_t)t0 * a.H + h) * HD;
  if (L > DEC_MAXK || (L + a.PS - 1) / a.PS > nb) {  // host contract broken: poison, never read wrong keys
    for (int d = tid; d < HD; d += DEC_NT) {
      o_s[d] = NAN;
      if (to_lds_only) continue;
      orow[d] = NAN;   // (and the packed copy the next GEMM reads, when armed)
      if (a.oph) xpack_store(a.oph, a.opl, t0, h * HD + d, NAN, a.prb);
    }
    __syncthreads();
    return false;
  }
  __syncthreads();
  const int kvh = h / (a.H / a.KVH);
  const size_t page_sz = (size_t)a.KVH * a.PS * HD, head_off = (size_t)kvh * a.PS * HD;
  // P.V layout: HD/4 lanes per key (one float4 of the V row each), 64/(HD/4) keys per wave-instruction,
  // the waves on interleaved keys.  The first NPF rounds of V rows are loaded here, in flight together
  // with the K rows, so the P.V pass after the softmax waits on no memory for up to 224-512 keys.
  constexpr int LPK = HD / 4, KPW = 64 / LPK, VSTR = DEC_NW * KPW;
  // (head_dim 128: 14 rounds, 224 keys -- with 16 the GQA launch below, which holds this body beside the multi-row
  // one, spills a VGPR)
  constexpr int NPF = HD == 128 ? 14 : (512 / VSTR < 16 ? 512 / VSTR : 16);
  const int sub = lane / LPK, l4 = lane % LPK;
  static_assert(KVB == 4 || KVB == 2 || KVB == 1, "cache element width");
  constexpr bool KV16 = KVB == 2, KV8 = KVB == 1;
  using kv_t = std::conditional_t<KV8, unsigned char, std::conditional_t<KV16, bf16_t, float>>;
  // 4 elements of a V row as loaded
  using v4_t = std::conditional_t<KV8, unsigned, std::conditional_t<KV16, uint2, float4>>;
  const kv_t* const kcp = reinterpret_cast<const kv_t*>(a.kc);
  const kv_t* const vcp = reinterpret_cast<const kv_t*>(a.vc);
  const size_t sc_page = (size_t)a.KVH * a.PS, sc_head = (size_t)kvh * a.PS;   // KV8: the scales' [page][kv head][slot]
  auto widen = [](v4_t v, [[maybe_unused]] float sc) {
    if constexpr (KV8) return fp8x4_to_f4(v, sc);
    else if constexpr (KV16) return bf4_to_f4(v);
    else return v;
  };
  v4_t vpf[NPF];
  float vsc[KV8 ? NPF : 1];   // KV8: the prefetched rows' scales
#pragma unroll
  for (int i = 0; i < NPF; ++i) {
    const int j = wave * KPW + sub + i * VSTR;
    if (j < L) {
      vpf[i] = *reinterpret_cast<const v4_t*>(vcp + (size_t)pg_s[j / a.PS] * page_sz + head_off +
                                              (size_t)(j % a.PS) * HD + 4 * l4);
      if constexpr (KV8) vsc[i] = a.vs[(size_t)pg_s[j / a.PS] * sc_page + sc_head + j % a.PS];
    }
  }
  auto dot4 = [&](float& s, int d, float4 k4) { s = dec_dot4(s, q_s + d, k4); };
  float mx = -INFINITY;
  for (int j = tid; j < L; j += DEC_NT) {
    const kv_t* kr = kcp + (size_t)pg_s[j / a.PS] * page_sz + head_off + (size_t)(j % a.PS) * HD;
    float s = 0.f;
    if constexpr (KV8) {
      static_assert(HD % 16 == 0, "decode attention on an FP8 cache: head_dim");
      const float sc = a.ks[(size_t)pg_s[j / a.PS] * sc_page + sc_head + j % a.PS];
#pragma unroll
      for (int d = 0; d < HD; d += 16) {
        const uint4 k16 = *reinterpret_cast<const uint4*>(kr + d);
        dot4(s, d, fp8x4_to_f4(k16.x, sc));
        dot4(s, d + 4, fp8x4_to_f4(k16.y, sc));
        dot4(s, d + 8, fp8x4_to_f4(k16.z, sc));
        dot4(s, d + 12, fp8x4_to_f4(k16.w, sc));
      }
    } else if constexpr (KV16) {
      static_assert(HD % 8 == 0, "decode attention on a bf16 cache: head_dim");
#pragma unroll
      for (int d = 0; d < HD; d += 8) {
        const uint4 k8 = *reinterpret_cast<const uint4*>(kr + d);
        dot4(s, d, bf4_to_f4(make_uint2(k8.x, k8.y)));
        dot4(s, d + 4, bf4_to_f4(make_uint2(k8.z, k8.w)));
      }
    } else {
#pragma unroll
      for (int d = 0; d < HD; d += 4) dot4(s, d, *reinterpret_cast<const float4*>(kr + d));
    }
    s_s[j] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  if (lane == 0) red_s[wave] = mx;
  __syncthreads();
  mx = red_s[0];
#pragma unroll
  for (int w = 1; w < DEC_NW; ++w) mx = fmaxf(mx, red_s[w]);
  float sum = 0.f;
  for (int j = tid; j < L; j += DEC_NT) {
    const float p = expf(s_s[j] - mx);
    s_s[j] = p;
    sum += p;
  }
  sum = block_sum<DEC_NW>(sum, red_s);  // its barriers also publish s_s
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  auto pv_add = [&](float p, float4 v) { dec_pv(acc, p, v); };
#pragma unroll
  for (int i = 0; i < NPF; ++i) {
    const int j = wave * KPW + sub + i * VSTR;
    if (j < L) pv_add(s_s[j], widen(vpf[i], vsc[KV8 ? i : 0]));
  }
#pragma unroll 8
  for (int j = wave * KPW + sub + NPF * VSTR; j < L; j += VSTR) {
    const float p = s_s[j];
    float sc = 0.f;
    if constexpr (KV8) sc = a.vs[(size_t)pg_s[j / a.PS] * sc_page + sc_head + j % a.PS];
    pv_add(p, widen(*reinterpret_cast<const v4_t*>(vcp + (size_t)pg_s[j / a.PS] * page_sz + head_off +
                                                   (size_t)(j % a.PS) * HD + 4 * l4), sc));
  }
  // the wave's keys, lanes LPK apart (lane_xor: no LDS round trip)
  auto xadd = [&](auto off) {
    constexpr int O = decltype(off)::value;
    if constexpr (O >= LPK && O < 64) {
      acc.x += lane_xor<O>(acc.x);
      acc.y += lane_xor<O>(acc.y);
      acc.z += lane_xor<O>(acc.z);
      acc.w += lane_xor<O>(acc.w);
    }
  };
  xadd(std::integral_constant<int, 8>{});
  xadd(std::integral_constant<int, 16>{});
  xadd(std::integral_constant<int, 32>{});
  if (sub == 0) *reinterpret_cast<float4*>(&acc_s[wave][4 * l4]) = acc;
  __syncthreads();
  for (int d = tid; d < HD; d += DEC_NT) {
    float o = 0.f;
#pragma unroll
    for (int w = 0; w < DEC_NW; ++w) o += acc_s[w][d];
    o_s[d] = o / sum;
    if (to_lds_only) continue;
    orow[d] = o / sum;
    if (a.oph) xpack_store(a.oph, a.opl, t0, h * HD + d, o / sum, a.prb);
  }
  __syncthreads();
  return true;
}

template <int HD, int KVB = 4>
__global__ __launch_bounds__(DEC_NT) void k_attn_decode(AttnArgs a) {
  static_assert(KVB != 1, "no FP8 form: only the AR speech decoder, whose cache stays fp32, takes this launch");
  __shared__ float o_s[HD];
  attn_decode_row<HD, KVB>(a, blockIdx.x, blockIdx.y, o_s, false);
}

// One-token GQA steps (the Qwen2 text step: 7 query heads per kv head, one token per session) on the grid of the
// multi-row kernel, (items, kv heads, split slots), with the path chosen per item on the device from the item's own
// key count -- a captured graph's launch serves a context as it grows:
//   L <= GQA_DEC_KEYS: slot z runs the single-row body above for query heads kvh * G + z, + nsplit, ... and stores out
//     (+ the packed copy) directly -- no MFMA layout staging, no partials, no ticket, and a result that does not
//     depend on nsplit / keys_per_split.  The text step's 16 slots give one head per workgroup; slots >= G leave
//     after the key count, as empty split slots do.
//   otherwise: attn_rows_body and its in-launch merge, unchanged.
// Every slot of an item reads the same L, so all of them take the same branch.  The two bodies' LDS sits side by
// side (77 + 22 KB; either body alone already runs one workgroup per CU).
// GQA_DEC_KEYS = 448, the measured crossover (scripts/attn_gqa_crossover.py, 8 sessions, 16 slots of 128 keys, graph
// replays, against k_attn_mfma<128, 8, 1> before this launch existed; profiles/gqa_decode_crossover.txt): 150 keys
// 7.3 against 13.9 us, 230 keys 9.1 / 14.0, 384 keys 12.4 / 14.6, 448 keys 14.4 / 15.0, 512 keys 15.7 / 15.2 -- the
// single-row body grows by ~2.4 us per 100 keys (one CU pulls a head's whole K / V), the split body by ~0.4.
constexpr int GQA_DEC_KEYS = 448;
static_assert(GQA_DEC_KEYS <= DEC_NT, "the single-row body scores one key per thread");
// KVB 2 (a bf16 cache): both bodies' bf16 forms, 44 + 22 KB of LDS; the crossover is kept.
// KVB 1 (an FP8 cache): both bodies' FP8 forms, the same LDS; the crossover is kept.
template <int HD, int KVB = 4>
__global__ __launch_bounds__(DEC_NT) void k_attn_gqa_decode(AttnArgs a) {
  static_assert(DEC_NW == 8, "shares the 8-wave multi-row body's block");
  __shared__ float o_s[HD];
  const int it = blockIdx.x, kvh = blockIdx.y, sp = blockIdx.z;
  const int L = a.tok_nvis[a.items ? a.items[3 * it + 1] : it];
  if (L <= GQA_DEC_KEYS) {
    const int G = a.H / a.KVH;
    for (int g = sp; g < G; g += a.nsplit) {
      // (a per-iteration copy of the page size: the body's per-lane address arithmetic, all derived from it, is then
      // computed inside the iteration; hoisted out of the loop it costs 54 spilled VGPRs)
      AttnArgs b = a;
      asm volatile("" : "+s"(b.PS));
      attn_decode_row<HD, KVB>(b, it, kvh * G + g, o_s, false);
    }
    return;
  }
  attn_rows_body<HD, DEC_NW, 1, false, KVB>(a, it, kvh, sp);
}

// The AR speech decoder's attention fused with its o projection, residual add and the next RMSNorm's statistics
// (models/decoder/decoder.py:341-349 through LlamaAttention.o_proj + the residual of LlamaDecoderLayer): o is a
// sum over heads, o[s] = sum_h att[s][h] . Wo[:, h*HD:(h+1)*HD]^T, so each (session, head) workgroup multiplies its
// own attention row by its head's slice of the packed o weight (N x HD, loaded into registers at the start, while the
// attention runs) and publishes an N-wide partial; the last head to arrive for a session (agent-scope release /
// acquire ticket, as the split merge) sums the H partials in head order (deterministic), adds the residual and
// writes x (in place), yg = x * gamma_next and the row's sum of squares (one statistics group) -- the next
// gate/up GEMM's RMSNorm-on-load input.  Workgroups of one head are dealt to one XCD (its L2 serves the head's
// slice to every session).  For o slices of <= 128 KiB per head (the 896-wide decoder; not Qwen2's 3584 x 128).
struct AttnOArgs {
  const bf16x8* wo;   // packed [N/16][K/32][64][8], K = H * HD
  float* part;        // [S][H][N]
  int* tickets;       // [S] zeroed, left zeroed
  float* x;           // [S][ldx] residual stream, updated in place
  const float* gnext; // [N]
  float* yg;          // [S][ldx]
  float* sout;        // [S]
  int N, ldx, KS;     // KS = K / 32
};
constexpr int AO_TILES = 8;   // 16-column tiles per wave (8 waves: up to 128 * 8 = 1024 columns)
template <int HD>
__global__ __launch_bounds__(DEC_NT) void k_attn_decode_o(AttnArgs a, AttnOArgs o) {
  constexpr int KPH = HD / 32;   // k-steps per head
  __shared__ float o_s[HD];
  __shared__ float red_s[DEC_NW];
  __shared__ int last_s;
  const int S = gridDim.x / (8 * ((a.H + 7) / 8));
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int h = xcd + 8 * (slot / S), it = slot % S;
  if (h >= a.H) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ntiles = (o.N + 15) / 16;
  // this head's o weight fragments: wave w owns tiles w*AO_TILES .. +AO_TILES, both of the head's k-steps
  bf16x8 wf[AO_TILES][KPH];
#pragma unroll
  for (int t = 0; t < AO_TILES; ++t) {
    const int tile = wave * AO_TILES + t;
#pragma unroll
    for (int k = 0; k < KPH; ++k)
      if (tile < ntiles) wf[t][k] = __builtin_nontemporal_load(o.wo + ((size_t)tile * o.KS + h * KPH + k) * 64 + lane);
  }
  attn_decode_row<HD>(a, it, h, o_s, true);
  // A fragments of the attention row (row 0 of a 16-row block; the other rows zero), fp32 split into hi + lo
  bf16x8 ah[KPH], al[KPH];
#pragma unroll
  for (int k = 0; k < KPH; ++k) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = (lane & 15) == 0 ? o_s[k * 32 + 8 * (lane >> 4) + e] : 0.f;
      const __bf16 hv = (__bf16)v;
      ah[k][e] = hv;
      al[k][e] = (__bf16)(v - (float)hv);
    }
  }
  const int s = a.items ? a.items[3 * it + 1] : it;   // this item's token (decode: one per sequence)
  float* prow = o.part + ((size_t)s * a.H + h) * o.N;
#pragma unroll
  for (int t = 0; t < AO_TILES; ++t) {
    const int tile = wave * AO_TILES + t;
    if (tile >= ntiles) break;   // wave-uniform
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KPH; ++k) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[k], wf[t][k], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[k], wf[t][k], acc, 0, 0, 0);
    }
    const int n = tile * 16 + lane;
    if (lane < 16 && n < o.N) prow[n] = acc[0];   // D row 0: lanes 0..15, element 0
  }
  // publish the partial and take the session's ticket (the split-merge protocol of attn_arrive_and_merge)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int old = __hip_atomic_fetch_add(o.tickets + s, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = old == a.H - 1;
  }
  __syncthreads();
  if (!last_s) return;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(o.tickets + s, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const float* ps = o.part + (size_t)s * a.H * o.N;
  float ssq = 0.f;
  for (int n = tid; n < o.N; n += DEC_NT) {
    // the H partials come from other XCDs' workgroups (a memory-side round trip each): all loads of a group of 16
    // heads are issued together, then summed in head order (deterministic)
    float v = 0.f;
    for (int h0 = 0; h0 < a.H; h0 += 16) {
      float pv[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) pv[j] = h0 + j < a.H ? ps[(size_t)(h0 + j) * o.N + n] : 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) v += pv[j];
    }
    const size_t off = (size_t)s * o.ldx + n;
    const float y = o.x[off] + v;
    o.x[off] = y;
    o.yg[off] = y * o.gnext[n];
    ssq += y * y;
  }
  ssq = block_sum<DEC_NW>(ssq, red_s);
  if (tid == 0) o.sout[s] = ssq;
}

// merge split partials: grid (T, H)
__global__ void k_attn_combine(AttnArgs a, int hd) {
  const int t = blockIdx.x, h = blockIdx.y;
  const size_t base = ((size_t)t * a.H + h) * a.nsplit;
  float M = -INFINITY;
  for (int s = 0; s < a.nsplit; ++s)
    if (a.part_ml[(base + s) * 2 + 1] > 0.f) M = fmaxf(M, a.part_ml[(base + s) * 2]);
  float l = 0.f;
  for (int s = 0; s < a.nsplit; ++s) {
    const float ls = a.part_ml[(base + s) * 2 + 1];
    if (ls > 0.f) l += ls * expf(a.part_ml[(base + s) * 2] - M);
  }
  for (int dd = threadIdx.x; dd < hd; dd += blockDim.x) {
    float o = 0.f;
    for (int s = 0; s < a.nsplit; ++s) {
      const float ls = a.part_ml[(base + s) * 2 + 1];
      if (ls > 0.f) o += a.part_o[(base + s) * hd + dd] * expf(a.part_ml[(base + s) * 2] - M);
    }
    a.out[((size_t)t * a.H + h) * hd + dd] = o / l;
  }
}

// ------------------------------------------------------------------ encoder rel-pos attention
__global__ void k_enc_kv_write(const float* k, const float* v, int ldkv, int B, int T, int d, const int* start,
                               const int* len, const int* ring, int cap, float* kr, float* vr) {
  const long long total = (long long)B * T * d;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % d);
    const int i = (int)((e / d) % T);
    const int b = (int)(e / ((long long)T * d));
    const int slot = (start[b] + len[b] + i) % cap;
    const size_t rb = ring ? (size_t)ring[b] : (size_t)b;
    kr[(rb * cap + slot) * d + c] = k[((size_t)b * T + i) * ldkv + c];
    vr[(rb * cap + slot) * d + c] = v[((size_t)b * T + i) * ldkv + c];
  }
}

template <int TMAX, int LMAX>
__global__ __launch_bounds__(256) void k_relpos_attn(const float* q, int ldq, const float* kr, const float* vr,
                                                     int cap, const int* start, const int* len, const int* ring,
                                                     const float* ptab,
                                                     const int* pstart, const float* bu, const float* bv, int T,
                                                     int h, int dk, float scale, float* out, int ldo) {
  extern __shared__ float smem[];
  float* qu = smem;                     // [T][dk]
  float* qv = qu + TMAX * dk;           // [T][dk]
  float* sc = qv + TMAX * dk;           // [T][LMAX]
  const int b = blockIdx.x, hh = blockIdx.y;
  const int d = h * dk;
  const size_t rb = ring ? (size_t)ring[b] : (size_t)b;
  const int Lk = len[b] + T;
  const int st = start[b];
  const int ps = pstart[b];
  for (int e = threadIdx.x; e < T * dk; e += blockDim.x) {
    const int i = e / dk, c = e % dk;
    const float x = q[((size_t)b * T + i) * ldq + hh * dk + c];
    qu[i * dk + c] = x + bu[hh * dk + c];
    qv[i * dk + c] = x + bv[hh * dk + c];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < T * Lk; e += blockDim.x) {
    const int i = e / Lk, j = e % Lk;
    const int slot = (st + j) % cap;
    const float* kk = kr + (rb * cap + slot) * d + hh * dk;
    const float* pp = ptab + (size_t)(ps + j) * d + hh * dk;
    float s1 = 0.f, s2 = 0.f;
    for (int c = 0; c < dk; ++c) {
      s1 += qu[i * dk + c] * kk[c];
      s2 += qv[i * dk + c] * pp[c];
    }
    sc[i * LMAX + j] = (s1 + s2) * scale;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < T; i += blockDim.x / 64) {
    float m = -INFINITY;
    for (int j = lane; j < Lk; j += 64) m = fmaxf(m, sc[i * LMAX + j]);
    m = wave_max(m);
    float s = 0.f;
    for (int j = lane; j < Lk; j += 64) {
      const float e = expf(sc[i * LMAX + j] - m);
      sc[i * LMAX + j] = e;
      s += e;
    }
    s = wave_sum(s);
    const float r = 1.f / s;
    for (int j = lane; j < Lk; j += 64) sc[i * LMAX + j] *= r;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < T * dk; e += blockDim.x) {
    const int i = e / dk, c = e % dk;
    float acc = 0.f;
    for (int j = 0; j < Lk; ++j) {
      const int slot = (st + j) % cap;
      acc += sc[i * LMAX + j] * vr[(rb * cap + slot) * d + hh * dk + c];
    }
    out[((size_t)b * T + i) * ldo + hh * dk + c] = acc;
  }
}

// Rel-pos attention of one chunk for one (user, head) out of LDS, the body of both encoder kernels below: every key /
// value / position row this head needs is staged in LDS with 16-B coalesced loads; scores, softmax and P.V then run
// out of LDS (MultiHeadedAttention.infer, models/encoder/attention.py:415-428).  The caller resolves the work group's
// ring slot rb, ring start st, rows Lold already in the ring (Lold + T <= cap, which the host cannot check: the
// engine's cap is its buffersize + the largest T), position start ps and first q|k|v row row0.
//   fused   (CHUNKS = false, k_relpos_fused): a context row is in the ring or is one of the chunk's own q|k|v rows;
//           the new rows are appended to the ring while staging (the cat-and-trim), and the output is also written
//           packed when oph is set.
//   grouped (CHUNKS = true, k_relpos_chunks): chunk jc of a group whose q|k|v rows are chunk-major (row
//           (jc * B + b) * T + i); a context row is in the ring as it was before the launch, one of the chunk's own
//           rows, or a row of an earlier chunk of the group.  The ring is neither written nor read where the group
//           will append (k_relpos_chunks_append does that afterwards); no packed output.
template <bool CHUNKS>
__device__ __forceinline__ void relpos_body(const float* qkv, int ldq, float* kr, float* vr, int cap, size_t rb, int st,
                                            int Lold, int ps, size_t row0, int jc, int B, const float* ptab,
                                            const float* bu, const float* bv, int T, int h, int dk, float scale,
                                            float* out, int ldo, uint16_t* oph, uint16_t* opl, int prb) {
  extern __shared__ float smem[];
  const int KP = dk + 4;  // padded rows: lanes on consecutive keys hit distinct banks
  float* k_s = smem;                  // [cap][KP]
  float* v_s = k_s + cap * KP;        // [cap][KP]
  float* p_s = v_s + cap * KP;        // [cap][KP]
  float* qu = p_s + cap * KP;         // [T][dk]
  float* qv = qu + T * dk;            // [T][dk]
  float* sc = qv + T * dk;            // [T][cap]
  const int b = blockIdx.x, hh = blockIdx.y;
  const int d = h * dk;
  const int Lk = Lold + T;
  const int D4 = dk / 4;
  typedef float v4f __attribute__((ext_vector_type(4)));   // (a native vector: the arrays stay in VGPRs)
  // staging: each thread's key / value / position rows (up to RB_ per batch) are all loaded before any of them
  // is stored to LDS -- one dependent memory round trip per batch instead of one per row
  constexpr int RB_ = 8;
  // the chunk's query rows (+ the u / v position biases), at most 2 per thread, ride in the first batch
  float qx[2], qbu[2], qbv[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int e = threadIdx.x + r * 256;
    const int i = e < T * dk ? e / dk : 0, c = e < T * dk ? e % dk : 0;
    qx[r] = qkv[(row0 + i) * ldq + hh * dk + c];
    qbu[r] = bu[hh * dk + c];
    qbv[r] = bv[hh * dk + c];
  }
  for (int e0 = 0; e0 < Lk * D4; e0 += RB_ * 256) {
    v4f kk[RB_], vv[RB_], pp[RB_];
#pragma unroll
    for (int q = 0; q < RB_; ++q) {
      const int e = e0 + q * 256 + threadIdx.x;
      const bool on = e < Lk * D4;
      const int j = on ? e / D4 : 0, c = on ? (e % D4) * 4 : 0;
      if constexpr (CHUNKS) {
        // row j of the context: the chunk's own (j >= Lold), one an earlier chunk of this launch appended (age <
        // jc * T), or one in the ring from before the launch
        const int age = Lold - 1 - j;
        const float* src;
        const float* ksrc;
        const float* vsrc;
        if (j >= Lold) {
          src = qkv + (row0 + (j - Lold)) * ldq + hh * dk + c;
          ksrc = src + d;
          vsrc = src + 2 * d;
        } else if (age < jc * T) {
          const int jj = jc - 1 - age / T, t = T - 1 - age % T;
          src = qkv + (((size_t)jj * B + b) * T + t) * ldq + hh * dk + c;
          ksrc = src + d;
          vsrc = src + 2 * d;
        } else {
          const size_t ro = (rb * cap + (st + j) % cap) * d + hh * dk + c;
          ksrc = kr + ro;
          vsrc = vr + ro;
        }
        kk[q] = *reinterpret_cast<const v4f*>(ksrc);
        vv[q] = *reinterpret_cast<const v4f*>(vsrc);
      } else {   // branch-free: the chunk's new rows come from the q|k|v output through the same loads
        const bool old_row = j < Lold;
        const size_t ro = (rb * cap + (st + j) % cap) * d + hh * dk + c;
        const float* src = qkv + (row0 + (old_row ? 0 : j - Lold)) * ldq + hh * dk + c;
        kk[q] = *reinterpret_cast<const v4f*>(old_row ? kr + ro : src + d);
        vv[q] = *reinterpret_cast<const v4f*>(old_row ? vr + ro : src + 2 * d);
      }
      pp[q] = *reinterpret_cast<const v4f*>(ptab + (size_t)(ps + j) * d + hh * dk + c);
    }
#pragma unroll
    for (int q = 0; q < RB_; ++q) {
      const int e = e0 + q * 256 + threadIdx.x;
      if (e < Lk * D4) {
        const int j = e / D4, c = (e % D4) * 4;
        if constexpr (!CHUNKS) {
          if (j >= Lold) {   // the chunk's new rows enter the ring
            const size_t ro = (rb * cap + (st + j) % cap) * d + hh * dk + c;
            *reinterpret_cast<v4f*>(kr + ro) = kk[q];
            *reinterpret_cast<v4f*>(vr + ro) = vv[q];
          }
        }
        *reinterpret_cast<v4f*>(k_s + j * KP + c) = kk[q];
        *reinterpret_cast<v4f*>(v_s + j * KP + c) = vv[q];
        *reinterpret_cast<v4f*>(p_s + j * KP + c) = pp[q];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int e = threadIdx.x + r * 256;
    if (e < T * dk) {
      qu[e] = qx[r] + qbu[r];
      qv[e] = qx[r] + qbv[r];
    }
  }
  for (int e = threadIdx.x + 512; e < T * dk; e += blockDim.x) {   // (T * dk > 512: not used at dk 64, T <= 8)
    const int i = e / dk, c = e % dk;
    const float x = qkv[(row0 + i) * ldq + hh * dk + c];
    qu[i * dk + c] = x + bu[hh * dk + c];
    qv[i * dk + c] = x + bv[hh * dk + c];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < T * Lk; e += blockDim.x) {
    const int i = e / Lk, j = e % Lk;
    const float* kk = k_s + j * KP;
    const float* pp = p_s + j * KP;
    const float* a1 = qu + i * dk;
    const float* a2 = qv + i * dk;
    float s1 = 0.f, s2 = 0.f;
    for (int c = 0; c < dk; c += 4) {
      const float4 k4 = *reinterpret_cast<const float4*>(kk + c), p4 = *reinterpret_cast<const float4*>(pp + c);
      const float4 u4 = *reinterpret_cast<const float4*>(a1 + c), w4 = *reinterpret_cast<const float4*>(a2 + c);
      s1 += u4.x * k4.x + u4.y * k4.y + u4.z * k4.z + u4.w * k4.w;
      s2 += w4.x * p4.x + w4.y * p4.y + w4.z * p4.z + w4.w * p4.w;
    }
    sc[i * cap + j] = (s1 + s2) * scale;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < T; i += blockDim.x / 64) {
    float m = -INFINITY;
    for (int j = lane; j < Lk; j += 64) m = fmaxf(m, sc[i * cap + j]);
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < Lk; j += 64) {
      const float e = expf(sc[i * cap + j] - m);
      sc[i * cap + j] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    const float r = 1.f / sum;
    for (int j = lane; j < Lk; j += 64) sc[i * cap + j] *= r;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < T * dk; e += blockDim.x) {
    const int i = e / dk, c = e % dk;
    const float* pr = sc + i * cap;
    float acc = 0.f;
    for (int j = 0; j < Lk; ++j) acc += pr[j] * v_s[j * KP + c];
    out[(row0 + i) * ldo + hh * dk + c] = acc;
    if constexpr (!CHUNKS) {
      if (oph) xpack_store(oph, opl, (int)row0 + i, hh * dk + c, acc, prb);   // the out projection's packed input
    }
  }
}

// Fused ring append + rel-pos attention of one chunk, one work group per (user, head): relpos_body's fused form.
__global__ __launch_bounds__(256) void k_relpos_fused(const float* qkv, int ldq, float* kr, float* vr, int cap,
                                                      const int* start, const int* len, const int* ring,
                                                      const float* ptab, const int* pstart, const float* bu,
                                                      const float* bv, int T, int h, int dk, float scale, float* out,
                                                      int ldo, uint16_t* oph, uint16_t* opl, int prb) {
  const int b = blockIdx.x;
  relpos_body<false>(qkv, ldq, kr, vr, cap, ring ? (size_t)ring[b] : (size_t)b, start[b], len[b], pstart[b],
                     (size_t)b * T, 0, 0, ptab, bu, bv, T, h, dk, scale, out, ldo, oph, opl, prb);
}

// C consecutive chunks of the same users in ONE launch (the offline listen's grouped encoder,
// SpeechEncoderEngine.run(chunks=C)), one work group per (user, head, chunk), all chunks at once: relpos_body's
// grouped form with chunk jc's metadata (meta[jc][start B | len B | ring B | pstart B]: host_meta after the chunks
// before it).  Chunk jc sees exactly the left context the sequential per-chunk launches give it.
__global__ __launch_bounds__(256) void k_relpos_chunks(const float* qkv, int ldq, float* kr, float* vr, int cap,
                                                       const int* meta, int B, int C, const float* ptab,
                                                       const float* bu, const float* bv, int T, int h, int dk,
                                                       float scale, float* out, int ldo) {
  const int b = blockIdx.x, jc = blockIdx.z;
  const int* m = meta + (size_t)jc * 4 * B;
  relpos_body<true>(qkv, ldq, kr, vr, cap, (size_t)m[2 * B + b], m[b], m[B + b], m[3 * B + b],
                    ((size_t)jc * B + b) * T, jc, B, ptab, bu, bv, T, h, dk, scale, out, ldo, nullptr, nullptr, 0);
}

// The ring appends of a listen group's C chunks, after k_relpos_chunks has read the ring: chunk j's T rows (k, v
// columns of its q|k|v rows) at its sequential positions (start_j + len_j + t) % cap -- consecutive over the chunks, so
// the ring ends as C sequential appends leave it (C * T <= cap).
__global__ void k_relpos_chunks_append(const float* qkv, int ldq, float* kr, float* vr, int cap, const int* meta, int B,
                                       int C, int T, int d) {
  const int D4 = d / 4;
  const long long n = (long long)C * B * T * D4;
  typedef float v4f __attribute__((ext_vector_type(4)));
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % D4) * 4;
    const long long r = e / D4;          // q|k|v row: (jc * B + b) * T + t
    const int t = (int)(r % T);
    const int b = (int)((r / T) % B);
    const int jc = (int)(r / ((long long)T * B));
    const int* m = meta + (size_t)jc * 4 * B;
    const size_t rb = (size_t)m[2 * B + b];
    const size_t ro = (rb * cap + (m[b] + m[B + b] + t) % cap) * d + c;
    const float* src = qkv + (size_t)r * ldq + c;
    *reinterpret_cast<v4f*>(kr + ro) = *reinterpret_cast<const v4f*>(src + d);
    *reinterpret_cast<v4f*>(vr + ro) = *reinterpret_cast<const v4f*>(src + 2 * d);
  }
}

// waves per work group of the multi-row MFMA attention at head_dim 128 (the Qwen2 listen / text rows): 8 (default:
// 128-key tiles, so a 128-key split loads in one round instead of two) or 4 (64-key tiles); FO_ATTN_NW.  r03t
// (scripts/attn_kps_sweep.py, 8 sessions, graph-replayed): 2 tokens x 200 keys 18.0 -> 15.2 us, 400 keys 21.2 ->
// 17.7 us, 1 token x 200 keys 15.9 -> 13.8 us (profiles/r03t_attn_nw_ab.txt)
int g_attn_nw = -1;
inline int attn_waves() {
  if (g_attn_nw < 0) {
    const char* e = getenv("FO_ATTN_NW");
    g_attn_nw = (e && atoi(e) == 4) ? 4 : 8;   // (16 waves: 128 VGPRs a lane, 109 spilled -- not built)
  }
  return g_attn_nw;
}
thread_local unsigned long long* g_attn_trc = nullptr;   // fo_attention_set_trace (probes)

// query rows one attention work item may carry (fo_attn_max_rows): 32 on the 8-wave head-dim-128 kernel
inline int attn_max_rows(int hd) { return hd == 128 && attn_waves() == 8 ? 32 : 16; }

// fo_attention_set_opack: the next launch's packed output and its extent (columns, allocated row blocks)
thread_local uint16_t* g_oph = nullptr;
thread_local uint16_t* g_opl = nullptr;
thread_local int g_op_cols = 0, g_op_rb = 0;

// The armed packed output, taken and disarmed: the launch that takes it consumes it whatever happens.
struct OPack {
  uint16_t *hi, *lo;
  int cols, rb;
};
inline OPack take_opack() {
  const OPack o{g_oph, g_opl, g_op_cols, g_op_rb};
  g_oph = g_opl = nullptr;
  g_op_cols = g_op_rb = 0;
  return o;
}

// Dynamic LDS of relpos_body: k_s / v_s / p_s [cap][dk + 4], qu / qv [T][dk], sc [T][cap] floats; refused for the
// entry `fn` past 160 KiB.
inline int relpos_lds(const char* fn, int cap, int T, int dk, size_t* lds) {
  *lds = (size_t)(3 * cap * (dk + 4) + 2 * T * dk + T * cap) * sizeof(float);
  FO_REQUIRE(*lds <= 160 * 1024, "%s: ring of %d x %d exceeds LDS", fn, cap, dk);
  return 0;
}

// the launch counters of the FP8 KV cache (fo_kv8_counts): fo_kv8_append, fo_attention_kv8
std::atomic<long long> g_kv8_launches[2];

inline int grid_for(long long n) {
  long long g = (n + 255) / 256;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

// The multi-row launch over a cache of KVB-byte elements (4: fp32, 2: bf16, 1: e4m3): 8 waves at head dim 128, with
// two row tiles past 16 query rows; 4 waves at 64 and 32.
template <int KVB>
void launch_rows(int hd, int max_rows, dim3 grid, const AttnArgs& a, hipStream_t s) {
  if (hd == 128 && max_rows > 16) hipLaunchKernelGGL((k_attn_mfma<128, 8, 2, false, KVB>), grid, dim3(512), 0, s, a);
  else if (hd == 128) hipLaunchKernelGGL((k_attn_mfma<128, 8, 1, false, KVB>), grid, dim3(512), 0, s, a);
  else if (hd == 64) hipLaunchKernelGGL((k_attn_mfma<64, 4, 1, false, KVB>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_attn_mfma<32, 4, 1, false, KVB>), grid, dim3(256), 0, s, a);
}

// The single-row decode launch over a cache of KVB-byte elements (4: fp32, 2: bf16).
template <int KVB>
void launch_decode(int hd, dim3 grid, const AttnArgs& a, hipStream_t s) {
  if (hd == 128) hipLaunchKernelGGL((k_attn_decode<128, KVB>), grid, dim3(DEC_NT), 0, s, a);
  else if (hd == 64) hipLaunchKernelGGL((k_attn_decode<64, KVB>), grid, dim3(DEC_NT), 0, s, a);
  else hipLaunchKernelGGL((k_attn_decode<32, KVB>), grid, dim3(DEC_NT), 0, s, a);
}

}  // namespace

extern "C" {

int fo_attention_set_opack(void* hi, void* lo, int cols, int cap_rb) {
  g_oph = g_opl = nullptr;
  g_op_cols = g_op_rb = 0;
  FO_REQUIRE((hi == nullptr) == (lo == nullptr), "fo_attention_set_opack: both halves or neither");
  if (!hi) return 0;
  FO_REQUIRE(cols > 0 && (cols & 31) == 0 && cap_rb >= 1 && cap_rb <= 4,
             "fo_attention_set_opack: cols %d (a multiple of 32) and 1..4 row blocks (%d) required", cols, cap_rb);
  g_oph = reinterpret_cast<uint16_t*>(hi);
  g_opl = reinterpret_cast<uint16_t*>(lo);
  g_op_cols = cols;
  g_op_rb = cap_rb;
  return 0;
}

// Decode attention (one token per sequence, items NULL or one per token) fused with the o projection + residual
// + next-norm statistics (k_attn_decode_o above).  Arguments as fo_attention's decode form, plus: wo packed o weight
// (N x H*hd), part >= T * H * N floats, tickets T zeroed ints (left zeroed), x [T][ldx] residual (updated), gnext
// [N], yg [T][ldx], sout [T] (one statistics group per row).
int fo_attention_o_kv(const float* q, int T, const int* items, const int* tok_nvis, const int* block_table, int maxb,
                      int PS, const void* kc, const void* vc, int H, int hd, float scale, const void* wo, int N,
                      float* part, int* tickets, float* x, int ldx, const float* gnext, float* yg, float* sout,
                      int kv_bytes, hipStream_t s) {
  FO_REQUIRE(kv_bytes == 4 || kv_bytes == 2, "fo_attention_o: kv_bytes %d (4 = fp32, 2 = bf16)", kv_bytes);
  FO_REQUIRE(kv_bytes == 4, "fo_attention_o: the attention fused with the o projection reads an fp32 cache only (no "
                            "bf16 form of k_attn_decode_o)");
  FO_REQUIRE(T > 0 && H > 0 && hd == 64 && N > 0 && N <= 16 * AO_TILES * DEC_NW && ldx >= N,
             "fo_attention_o: T=%d H=%d hd=%d N=%d (N <= %d)", T, H, hd, N, 16 * AO_TILES * DEC_NW);
  FO_REQUIRE((long long)maxb * PS <= DEC_MAXK, "fo_attention_o: %d keys per sequence exceed %d", maxb * PS, DEC_MAXK);
  FO_REQUIRE(wo && part && tickets && x && gnext && yg && sout, "fo_attention_o: null argument");
  AttnArgs a{q, items, tok_nvis, block_table, kc, vc, nullptr, nullptr, nullptr, H, H, PS, maxb, 1, scale,
             nullptr, 0, 1, nullptr, nullptr, 1};
  AttnOArgs o{reinterpret_cast<const bf16x8*>(wo), part, tickets, x, gnext, yg, sout, N, ldx, H * hd / 32};
  const int grid = 8 * T * ((H + 7) / 8);
  hipLaunchKernelGGL((k_attn_decode_o<64>), dim3(grid), dim3(DEC_NT), 0, s, a, o);
  fo::count_launch(FO_L_ATTN_O);
  return fo::check_launch("fo_attention_o");
}

int fo_attention_o(const float* q, int T, const int* items, const int* tok_nvis, const int* block_table, int maxb,
                   int PS, const float* kc, const float* vc, int H, int hd, float scale, const void* wo, int N,
                   float* part, int* tickets, float* x, int ldx, const float* gnext, float* yg, float* sout,
                   hipStream_t s) {
  return fo_attention_o_kv(q, T, items, tok_nvis, block_table, maxb, PS, kc, vc, H, hd, scale, wo, N, part, tickets, x,
                           ldx, gnext, yg, sout, 4, s);
}

int fo_attn_max_rows(int hd) { return attn_max_rows(hd); }

int fo_attention_set_trace(void* trace) {
  g_attn_trc = reinterpret_cast<unsigned long long*>(trace);
  return 0;
}

int fo_attn_nsplit(int max_keys, int n_items, int KVH) {
  // enough work groups to cover the chip (~2 per CU) while every split keeps >= one 64-key tile
  const int by_keys = (max_keys + KT - 1) / KT;
  const int wgs = n_items * KVH;
  int ns = (512 + wgs - 1) / wgs;
  if (ns > by_keys) ns = by_keys;
  if (ns > 32) ns = 32;
  const int need = (max_keys + MAXPG * 16 - 1) / (MAXPG * 16);  // every split within the LDS page table
  if (ns < need) ns = need;
  return ns < 1 ? 1 : ns;
}

int fo_rope_kv_write_kv(const float* qkv, int ldq, int T, int H, int KVH, int hd, const int* pos, const int* slot,
                        const float* cos_t, const float* sin_t, float* q_out, void* kc, void* vc, int PS, int kv_bytes,
                        hipStream_t s) {
  FO_REQUIRE(T > 0 && (hd % 2) == 0, "fo_rope_kv_write: bad shape");
  FO_REQUIRE(kv_bytes == 4 || kv_bytes == 2, "fo_rope_kv_write: kv_bytes %d (4 = fp32, 2 = bf16)", kv_bytes);
  hipLaunchKernelGGL(k_rope_kv_write, dim3(T), dim3(256), 0, s, qkv, ldq, T, H, KVH, hd, pos, slot, cos_t, sin_t,
                     q_out, kc, vc, PS, kv_bytes == 2 ? 1 : 0, fo::kv_bf16_values());
  return fo::check_launch("fo_rope_kv_write");
}

int fo_rope_kv_write(const float* qkv, int ldq, int T, int H, int KVH, int hd, const int* pos, const int* slot,
                     const float* cos_t, const float* sin_t, float* q_out, float* kc, float* vc, int PS,
                     hipStream_t s) {
  return fo_rope_kv_write_kv(qkv, ldq, T, H, KVH, hd, pos, slot, cos_t, sin_t, q_out, kc, vc, PS, 4, s);
}

// q [T][H*hd] -> out [T][H*hd].  items [n_items][3] (sequence, first token, tokens), or NULL for a uniform batch
// (item b = sequence b = tokens b*T/n_items .. (b+1)*T/n_items - 1), with
// tokens * (H/KVH) <= max_rows <= 64; part_ml >= T*H*nsplit*2 and part_o >= T*H*nsplit*hd floats
// when nsplit > 1.  tickets (nullable): n_items*KVH zero-initialised ints; then each item takes
// min(nsplit, ceil(keys / keys_per_split)) splits and the last one merges them in this launch (the
// tickets are left zeroed); without tickets nsplit static splits are merged by a second launch.
int fo_attention(const float* q, int T, const int* items, int n_items, int max_rows, const int* tok_nvis,
                 const int* block_table, int maxb, int PS, const float* kc, const float* vc, int H, int KVH, int hd,
                 float scale, int nsplit, float* part_ml, float* part_o, float* out, int* tickets,
                 int keys_per_split, hipStream_t s) {
  return fo_attention_kv(q, T, items, n_items, max_rows, tok_nvis, block_table, maxb, PS, kc, vc, H, KVH, hd, scale,
                         nsplit, part_ml, part_o, out, tickets, keys_per_split, 4, s);
}

// The attention launch over a cache of kv_bytes-wide elements, for the entry `fn` (its name opens every refusal):
// 4: fp32, 2: bf16; kv8 (fo_attention_kv8 only): e4m3fn codes with the scales ks / vs
static int attention_any(const char* fn, const float* q, int T, const int* items, int n_items, int max_rows,
                         const int* tok_nvis, const int* block_table, int maxb, int PS, const void* kc, const void* vc,
                         const float* ks, const float* vs, int H, int KVH, int hd, float scale, int nsplit,
                         float* part_ml, float* part_o, float* out, int* tickets, int keys_per_split, int kv_bytes,
                         bool kv8, hipStream_t s) {
  const OPack op = take_opack();
  FO_REQUIRE(T > 0 && n_items > 0 && KVH > 0 && H % KVH == 0, "%s: bad shape", fn);
  FO_REQUIRE(!op.hi || (op.cols == H * hd && op.rb * 16 >= T),
             "%s: packed output of %d columns x %d row blocks armed for %d x %d tokens", fn, op.cols, op.rb,
             H * hd, T);
  FO_REQUIRE(items || T % n_items == 0, "%s: items NULL needs T / n_items tokens per item", fn);
  FO_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head_dim %d unsupported", fn, hd);
  FO_REQUIRE(kv8 || kv_bytes == 4 || kv_bytes == 2, "%s: kv_bytes %d (4 = fp32, 2 = bf16)", fn, kv_bytes);
  FO_REQUIRE(!kv8 || (kc && vc && ks && vs), "%s: NULL codes or scales", fn);
  FO_REQUIRE(PS > 0, "%s: page size %d", fn, PS);
  const bool kv16 = kv_bytes != 4;   // (narrow: bf16 or e4m3)
  // The multi-row forms built for an fp32 cache only -- the 4-wave and the traced one here, the 2-wave one at the rows
  // launch below -- are each named beside the refusal that keeps a narrow cache off them (by name, for every launch
  // of the entry: never run on the wrong element size); the rows launch picks among them before the common ladder.
  const bool nw4 = hd == 128 && attn_waves() == 4;                        // k_attn_mfma<128>
  const bool traced = g_attn_trc && hd == 128 && !nw4 && max_rows <= 16;  // k_attn_mfma<128, 8, 1, true>
  FO_REQUIRE(!kv16 || !g_attn_trc, "%s: the traced launches (fo_attention_set_trace) read an fp32 cache only", fn);
  FO_REQUIRE(!kv16 || !nw4, "%s: FO_ATTN_NW=4 at head_dim 128 (k_attn_mfma<128, 4>) reads an fp32 cache only", fn);
  // up to 32 query rows per item on the 8-wave head-dim-128 kernel (two row tiles share every K / V load: a duplex
  // tick's 4 tokens x 7 query heads per kv head read the session's keys once, not twice), 16 elsewhere
  const int rows_max = attn_max_rows(hd);
  FO_REQUIRE(max_rows >= 1 && max_rows <= rows_max, "%s: %d query rows per item (max %d)", fn, max_rows,
             rows_max);
  FO_REQUIRE(nsplit >= 1 && (nsplit == 1 || (part_ml && part_o)), "%s: bad split buffers", fn);
  FO_REQUIRE(!tickets || keys_per_split >= 32, "%s: keys_per_split %d < 32", fn, keys_per_split);
  // the in-launch merge reads the partials back through 32-bit buffer offsets (ld_sc1)
  FO_REQUIRE(!tickets || nsplit == 1 || (long long)T * H * nsplit * hd * 4 < (1ll << 31),
             "%s: %d tokens x %d heads x %d splits of partials exceed the merge's 2 GiB window", fn, T, H, nsplit);
  AttnArgs a{q, items, tok_nvis, block_table, kc, vc, part_ml, part_o, out, H, KVH, PS, maxb, nsplit, scale,
             tickets, keys_per_split, items ? 1 : T / n_items, op.hi, op.lo, (T + 15) / 16, g_attn_trc,
             g_attn_trc && getenv("FO_ATTN_TRACE_REPS") ? atoi(getenv("FO_ATTN_TRACE_REPS")) : 1, ks, vs};
  const bool dec = max_rows == 1 && (long long)maxb * PS <= DEC_MAXK;
  FO_REQUIRE(!a.oph || (T <= 64 && (dec || nsplit == 1 || tickets)),
             "%s: packed output needs <= 64 tokens and no combine launch", fn);
  FO_REQUIRE(!kv8 || !dec, "%s: one query row per item takes the single-row decode form (k_attn_decode), which has no "
                           "FP8 form (the AR speech decoder's cache stays fp32)", fn);
  if (dec) {  // one query row per (session, head): decode kernel
    dim3 g1(n_items, H);
    if (kv16) launch_decode<2>(hd, g1, a, s);
    else launch_decode<4>(hd, g1, a, s);
    fo::count_launch(FO_L_ATTN_DECODE);
    if (a.oph) fo::count_launch(FO_L_ATTN_OPACK);
    return fo::check_launch("fo_attention/decode");
  }
  dim3 grid(n_items, KVH, nsplit);
  // one token per item under GQA at head_dim 128 (the Qwen2 text step): the launch that picks the single-row body or
  // the multi-row one per item on the device (k_attn_gqa_decode).  Static splits without tickets end in
  // k_attn_combine, which would overwrite a directly stored row, so they keep the multi-row launch.
  const int G = H / KVH;
  const bool gqa_dec = hd == 128 && KVH < H && G <= 8 && max_rows == G && (items || T == n_items) &&
                       (tickets || nsplit == 1) && attn_waves() == 8 && !a.trc;
  if (gqa_dec) {
    if (kv8) hipLaunchKernelGGL((k_attn_gqa_decode<128, 1>), grid, dim3(DEC_NT), 0, s, a);
    else if (kv16) hipLaunchKernelGGL((k_attn_gqa_decode<128, 2>), grid, dim3(DEC_NT), 0, s, a);
    else hipLaunchKernelGGL((k_attn_gqa_decode<128, 4>), grid, dim3(DEC_NT), 0, s, a);
    fo::count_launch(FO_L_ATTN_GQA_DECODE);
    if (kv8) g_kv8_launches[1].fetch_add(1, std::memory_order_relaxed);
    if (a.oph) fo::count_launch(FO_L_ATTN_OPACK);
    return fo::check_launch("fo_attention/gqa_decode");
  }
  // splits under 64 keys (the text step's short contexts spread over more CUs: a split's K / V arrive at one CU's
  // memory parallelism) take the 2-wave form with 32-key tiles
  const bool small = hd == 128 && tickets && keys_per_split < 64 && max_rows <= 16 && !a.trc;   // k_attn_mfma<128, 2>
  FO_REQUIRE(!kv16 || !small, "%s: keys_per_split %d takes the 2-wave form (k_attn_mfma<128, 2>), which reads "
                              "an fp32 cache only; a bf16 or FP8 cache needs >= 64", fn, keys_per_split);
  if (small) hipLaunchKernelGGL((k_attn_mfma<128, 2>), grid, dim3(128), 0, s, a);
  else if (traced) hipLaunchKernelGGL((k_attn_mfma<128, 8, 1, true>), grid, dim3(512), 0, s, a);
  else if (nw4) hipLaunchKernelGGL((k_attn_mfma<128>), grid, dim3(256), 0, s, a);
  else if (kv8) launch_rows<1>(hd, max_rows, grid, a, s);
  else if (kv16) launch_rows<2>(hd, max_rows, grid, a, s);
  else launch_rows<4>(hd, max_rows, grid, a, s);
  if (kv8) g_kv8_launches[1].fetch_add(1, std::memory_order_relaxed);
  fo::count_launch(FO_L_ATTN_MFMA);
  if (a.oph) fo::count_launch(FO_L_ATTN_OPACK);
  int rc = fo::check_launch("fo_attention/rows");
  if (rc || nsplit == 1 || tickets) return rc;
  hipLaunchKernelGGL(k_attn_combine, dim3(T, H), dim3(hd < 64 ? 64 : hd), 0, s, a, hd);
  return fo::check_launch("fo_attention/combine");
}

int fo_attention_kv(const float* q, int T, const int* items, int n_items, int max_rows, const int* tok_nvis,
                    const int* block_table, int maxb, int PS, const void* kc, const void* vc, int H, int KVH, int hd,
                    float scale, int nsplit, float* part_ml, float* part_o, float* out, int* tickets,
                    int keys_per_split, int kv_bytes, hipStream_t s) {
  return attention_any("fo_attention", q, T, items, n_items, max_rows, tok_nvis, block_table, maxb, PS, kc, vc, nullptr,
                       nullptr, H, KVH, hd, scale, nsplit, part_ml, part_o, out, tickets, keys_per_split, kv_bytes, false,
                       s);
}

// fo_attention over an FP8 cache: e4m3fn codes kc / vc with the scales ks / vs
int fo_attention_kv8(const float* q, int T, const int* items, int n_items, int max_rows, const int* tok_nvis,
                     const int* block_table, int maxb, int PS, const void* kc, const void* vc, int H, int KVH, int hd,
                     float scale, int nsplit, float* part_ml, float* part_o, float* out, int* tickets,
                     int keys_per_split, const float* ks, const float* vs, hipStream_t s) {
  return attention_any("fo_attention_kv8", q, T, items, n_items, max_rows, tok_nvis, block_table, maxb, PS, kc, vc, ks,
                       vs, H, KVH, hd, scale, nsplit, part_ml, part_o, out, tickets, keys_per_split, 1, true, s);
}

// The FP8 cache's append (k_kv8_append): the T staged fp32 rows of K and V ([KVH][stage_rows][hd], row t = token t)
// quantised into the codes kc / vc and scales ks / vs at slot[t] (pages of PS slots).
int fo_kv8_append(const float* k_stage, const float* v_stage, int T, int KVH, int hd, int stage_rows, const int* slot,
                  int PS, void* kc, float* ks, void* vc, float* vs, hipStream_t s) {
  FO_REQUIRE(kc && vc && ks && vs, "fo_kv8_append: NULL codes or scales");
  FO_REQUIRE(k_stage && v_stage && slot, "fo_kv8_append: NULL staged rows or slot table");
  FO_REQUIRE(hd == 32 || hd == 64 || hd == 128, "fo_kv8_append: head_dim %d unsupported (32, 64, 128)", hd);
  FO_REQUIRE(PS > 0 && KVH > 0, "fo_kv8_append: page size %d, %d kv heads", PS, KVH);
  FO_REQUIRE(T >= 1 && T <= stage_rows, "fo_kv8_append: T=%d outside 1..%d stage rows", T, stage_rows);
  FO_REQUIRE((long long)T * KVH * 2 < (1ll << 31), "fo_kv8_append: T=%d x %d kv heads", T, KVH);
  hipLaunchKernelGGL(k_kv8_append, dim3((T * KVH * 2 + 3) / 4), dim3(256), 0, s, k_stage, v_stage, T, KVH, hd,
                     stage_rows, slot, PS, reinterpret_cast<unsigned char*>(kc), ks,
                     reinterpret_cast<unsigned char*>(vc), vs);
  g_kv8_launches[0].fetch_add(1, std::memory_order_relaxed);
  return fo::check_launch("fo_kv8_append");
}

int fo_kv8_counts(long long* out, int n) {
  for (int i = 0; out && i < n && i < 2; ++i) out[i] = g_kv8_launches[i].load(std::memory_order_relaxed);
  return 2;
}

int fo_kv8_counts_reset(void) {
  for (int i = 0; i < 2; ++i) g_kv8_launches[i].store(0, std::memory_order_relaxed);
  return 0;
}

int fo_enc_kv_write(const float* k, const float* v, int ldkv, int B, int T, int d, const int* start, const int* len,
                    const int* ring, int cap, float* kr, float* vr, hipStream_t s) {
  const long long n = (long long)B * T * d;
  hipLaunchKernelGGL(k_enc_kv_write, dim3(grid_for(n)), dim3(256), 0, s, k, v, ldkv, B, T, d, start, len, ring, cap,
                     kr, vr);
  return fo::check_launch("fo_enc_kv_write");
}

int fo_relpos_attention_fused(const float* qkv, int ldq, float* kr, float* vr, int cap, const int* start,
                              const int* len, const int* ring, const float* ptab, const int* pstart, const float* bu,
                              const float* bv, int B, int T, int h, int dk, float scale, float* out, int ldo,
                              hipStream_t s) {
  const OPack op = take_opack();
  FO_REQUIRE(!op.hi || (op.cols == h * dk && op.rb * 16 >= B * T),
             "fo_relpos_attention_fused: packed output of %d columns x %d row blocks armed for %d x %d rows", op.cols,
             op.rb, h * dk, B * T);
  FO_REQUIRE(T >= 1 && T <= cap && dk % 4 == 0 && (ldq % 4) == 0, "fo_relpos_attention_fused: T=%d dk=%d", T, dk);
  size_t lds;
  if (int rc = relpos_lds("fo_relpos_attention_fused", cap, T, dk, &lds)) return rc;
  hipLaunchKernelGGL(k_relpos_fused, dim3(B, h), dim3(256), lds, s, qkv, ldq, kr, vr, cap, start, len, ring, ptab,
                     pstart, bu, bv, T, h, dk, scale, out, ldo, op.hi, op.lo, (B * T + 15) / 16);
  fo::count_launch(FO_L_RELPOS);
  if (op.hi) fo::count_launch(FO_L_ATTN_OPACK);
  return fo::check_launch("fo_relpos_attention_fused");
}

int fo_relpos_attention_chunks(const float* qkv, int ldq, float* kr, float* vr, int cap, const int* meta, int B, int C,
                               const float* ptab, const float* bu, const float* bv, int T, int h, int dk, float scale,
                               float* out, int ldo, hipStream_t s) {
  FO_REQUIRE(B >= 1 && C >= 1 && T >= 1 && T <= cap && dk % 4 == 0 && (ldq % 4) == 0,
             "fo_relpos_attention_chunks: B=%d C=%d T=%d dk=%d", B, C, T, dk);
  FO_REQUIRE(C * T <= cap, "fo_relpos_attention_chunks: %d chunks of %d frames exceed the ring (%d)", C, T, cap);
  size_t lds;
  if (int rc0 = relpos_lds("fo_relpos_attention_chunks", cap, T, dk, &lds)) return rc0;
  hipLaunchKernelGGL(k_relpos_chunks, dim3(B, h, C), dim3(256), lds, s, qkv, ldq, kr, vr, cap, meta, B, C, ptab, bu,
                     bv, T, h, dk, scale, out, ldo);
  fo::count_launch(FO_L_RELPOS);
  int rc = fo::check_launch("fo_relpos_attention_chunks");
  if (rc) return rc;
  const long long n = (long long)C * B * T * (h * dk / 4);
  hipLaunchKernelGGL(k_relpos_chunks_append, dim3(grid_for(n)), dim3(256), 0, s, qkv, ldq, kr, vr, cap, meta, B, C, T,
                     h * dk);
  return fo::check_launch("fo_relpos_attention_chunks/append");
}

int fo_relpos_attention(const float* q, int ldq, const float* kr, const float* vr, int cap, const int* start,
                        const int* len, const int* ring, const float* ptab, const int* pstart, const float* bu,
                        const float* bv, int B, int T, int h, int dk, float scale, float* out, int ldo,
                        hipStream_t s) {
  FO_REQUIRE(T <= 8 && cap + T <= 264, "fo_relpos_attention: T=%d cap=%d too large", T, cap);
  const size_t lds = (size_t)(2 * 8 * dk + 8 * 264) * sizeof(float);
  FO_REQUIRE(lds <= 65536, "fo_relpos_attention: dk too large");
  hipLaunchKernelGGL((k_relpos_attn<8, 264>), dim3(B, h), dim3(256), lds, s, q, ldq, kr, vr, cap, start, len, ring,
                     ptab, pstart, bu, bv, T, h, dk, scale, out, ldo);
  return fo::check_launch("fo_relpos_attention");
}

}  // extern "C"
