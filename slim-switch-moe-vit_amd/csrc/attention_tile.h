// The tile vocabulary of the attention family (attention.hip, attention_skip.hip, attention_bwd.hip; head dim 64, 16-bit operands):
// the LDS layouts, the MFMA / conversion / packing helpers, the LDS-DMA staging, the fragment loads and the 8-byte-piece stores --
// and attn_fwd_body, THE one-pass forward (N <= 256) behind both attn_fwd_kernel and attn_varlen_kernel.
#pragma once
#include "smoe_common.h"
#include <type_traits>

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
constexpr int ATT_D = 64;
constexpr int ATT_THREADS = 256;

// ---- LDS images: row-major [row][64 x 16 bit] = 128 bytes per row ----------------------------------------------------------------
// row image (K in the forward; Q, K, V, dO in the backward): 16-byte chunk XOR-swizzled by (row>>1)&7 -> conflict-free ds_read_b128
// row reads, 2-way transposed reads
__device__ __forceinline__ int img_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
// V of the forward (read transposed only): 32-byte segment index (= 16-column block dt) XOR-swizzled by (row>>1)&3 -> the transposed
// reads of 8 consecutive rows hit 8 different 32-byte slots of the 256-byte bank row
__device__ __forceinline__ int v_lds_off(int row, int dt) { return row * 128 + ((dt ^ ((row >> 1) & 3)) << 5); }

// Staging an operand image by LDS DMA (global_load_lds, 1 KiB = 8 rows per wave-instruction), the swizzle carried by the source
// address (cdna_hip_programming.md rule 21): piece_off = where this lane's 16 bytes of the 8-row piece `pc` lie in a source whose
// rows are `stride` elements apart (elements from row 0; rows >= n duplicate row n - 1; VSEG: the v_lds_off layout instead of
// img_off's) -- operands that share rows and layout (q / k / v of a token) share it; stage_piece = the DMA of that piece.
template <bool VSEG>
__device__ __forceinline__ int64_t piece_off(int64_t stride, int n, int pc, int lane) {
  const int row = pc * 8 + (lane >> 3), pos = lane & 7;
  const int srow = row < n ? row : n - 1;
  const int c = VSEG ? ((((pos >> 1) ^ ((row >> 1) & 3)) << 1) | (pos & 1)) : (pos ^ ((row >> 1) & 7));
  return (int64_t)srow * stride + c * 8;
}
template <typename HT> __device__ __forceinline__ void stage_piece(char* img, int pc, const HT* src) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)(img + pc * 1024), 16, 0, 0);
}

// ---- MFMA 16x16x32 and the 16-bit conversions, by element type ---------------------------------------------------------------------
template <typename HT>
__device__ __forceinline__ f32x4 mma(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (std::is_same<HT, f16>::value)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

template <typename HT> __device__ __forceinline__ unsigned short to16(float v) {
  if constexpr (std::is_same<HT, f16>::value) return __builtin_bit_cast(unsigned short, (f16)v);
  else return f32_to_bf16(v);
}
template <typename HT> __device__ __forceinline__ float from16(unsigned short v) {
  if constexpr (std::is_same<HT, f16>::value) return (float)__builtin_bit_cast(f16, v);
  else return bf16_to_f32(v);
}
// 8 values rounded to 16 bit one by one, in element order.  The backward's P / dS operands use this form and must keep it: cvt8
// below looks interchangeable there but changes which multiplies hipcc fuses into the conversion, and with that the bits of dK / dQ.
template <typename HT> __device__ __forceinline__ u32x4 pack8(const f32x4& lo, const f32x4& hi) {
  u32x4 r;
  r[0] = (uint32_t)to16<HT>(lo[0]) | ((uint32_t)to16<HT>(lo[1]) << 16);
  r[1] = (uint32_t)to16<HT>(lo[2]) | ((uint32_t)to16<HT>(lo[3]) << 16);
  r[2] = (uint32_t)to16<HT>(hi[0]) | ((uint32_t)to16<HT>(hi[1]) << 16);
  r[3] = (uint32_t)to16<HT>(hi[2]) | ((uint32_t)to16<HT>(hi[3]) << 16);
  return r;
}
// ... and 4 / 8 values through a vector of 16-bit elements, which hipcc converts in pairs (v_cvt_pk_f16_f32, v_perm_b32: a third of
// pack8's VALU issues, and the forward is VALU-issue bound).  The same bits as pack8 for the same f32 inputs -- but where a multiply
// feeds the conversion, hipcc fuses the two differently in the two forms (v_fma_mixlo_f16 rounds once, see wave_row_affine in
// smoe_common.h), so which form a call site uses is part of its result: the forward and every output store convert in pairs, the
// backward's P / dS operands one by one (its dS also goes to LDS value by value).  cvt8 is two cvt4 on purpose: built as one 8-element
// vector the same conversions cost attn_fwd_long_kernel<bf16> 24 registers (140 instead of 116: past the 128 that let two of its
// workgroups share a CU at N <= 320).
template <typename HT> __device__ __forceinline__ u32x2 cvt4(const f32x4& v) {
  s16x4 t;
#pragma unroll
  for (int r = 0; r < 4; ++r) t[r] = (short)to16<HT>(v[r]);
  return __builtin_bit_cast(u32x2, t);
}
template <typename HT> __device__ __forceinline__ u32x4 cvt8(const f32x4& lo, const f32x4& hi) {
  const u32x2 a = cvt4<HT>(lo), b = cvt4<HT>(hi);
  return u32x4{a[0], a[1], b[0], b[1]};
}
// an all-ones operand fragment: as the A operand it sums the B operand over its 32 k-slots
template <typename HT> __device__ __forceinline__ u32x4 ones() {
  const uint32_t one2 = std::is_same<HT, f16>::value ? 0x3C003C00u : 0x3F803F80u;
  return u32x4{one2, one2, one2, one2};
}

// ---- fragment loads ----------------------------------------------------------------------------------------------------------------
// one transposed read (ds_read_b64_tr_b16) and the A operand two of them make: k-slot (g, j), j < 4 <-> the rows of `lo`, j >= 4 <-> `hi`
__device__ __forceinline__ s16x4 tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}
__device__ __forceinline__ u32x4 tr_join(const s16x4& lo, const s16x4& hi) {
  s16x8 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) { v[r] = lo[r]; v[4 + r] = hi[r]; }
  return __builtin_bit_cast(u32x4, v);
}
// ... out of a row image: [row = column idx of the 16-column block `cb`][k-slot (g, j)]: j < 4 <-> image rows r_lo + j, j >= 4 <->
// r_hi + (j - 4); the lane supplies row (r + tq), columns 16 cb + 4 tp .. + 3
__device__ __forceinline__ u32x4 tr_pair(const char* img, int r_lo, int r_hi, int cb, int tq, int tp) {
  const int chunk = 2 * cb + (tp >> 1), sub = (tp & 1) * 8;
  return tr_join(tr_read(img + img_off(r_lo + tq, chunk) + sub), tr_read(img + img_off(r_hi + tq, chunk) + sub));
}
// the row fragments of token min(16 qt + qi, n - 1) straight from memory (a B operand with the token on the lane): elements
// 8 g .. 8 g + 7 and 32 + 8 g .. 32 + 8 g + 7 of its 64
template <typename HT>
__device__ __forceinline__ void load_q(const HT* base, int64_t stride, int n, int qt, int qi, int g, u32x4& f0, u32x4& f1) {
  int qrow = qt * 16 + qi;
  if (qrow >= n) qrow = n - 1;
  const HT* qp = base + (int64_t)qrow * stride + g * 8;
  f0 = *reinterpret_cast<const u32x4*>(qp);
  f1 = *reinterpret_cast<const u32x4*>(qp + 32);
}

// ---- store one 16-token tile, times `scale`, as 8-byte pieces: lane (g, token) holds head-dim elements 16 dt + 4 g + r; p = the
//      token's row + 4 g -----------------------------------------------------------------------------------------------------------
template <typename HT> __device__ __forceinline__ void store_tile(HT* p, const f32x4 (&acc)[4], float scale = 1.0f) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    f32x4 t;
#pragma unroll
    for (int r = 0; r < 4; ++r) t[r] = acc[dt][r] * scale;
    *reinterpret_cast<u32x2*>(p + dt * 16) = cvt4<HT>(t);
  }
}

// ---- the one-pass forward (N <= 256): softmax(q k^T * scale) v for one (image, head) ------------------------------------------------
// One workgroup (4 waves); K and V of the head (len x 64, 16-bit) sit in LDS, every wave walks 16-query tiles.  Per tile, "key on
// the lane":
//   S^T = K Q^T      MFMA 16x16x32 with the K fragment as the A operand and the Q fragment as B: lane (g, q) ends up
//                    with the scores of query q against keys 16 kt + 4 g + r  (kt = key tile, r = 0..3)
//   softmax          per-lane over its 4*NT scores, then across the 4 lanes that share a query (xor 16, xor 32)
//   O^T = V^T P^T    the S^T accumulators, rounded to 16 bit, ARE the B operand (k-slot (g, j) <-> key
//                    32 ks + 16 (j>>2) + 4 g + (j&3)); the matching A operand is read from row-major V with
//                    ds_read_b64_tr_b16 (hardware transpose read), two reads per fragment
// so P never touches LDS and V is never transposed in memory.
//
// The rows are base[0 .. len) (`3 H 64` elements apart, q / k / v `H 64` apart), the outputs obase[0 .. len) (`H 64` apart), lse_row
// (may be null) takes log2 of the normaliser per query.  NKT = key tiles of 16 held in LDS (compile-time, >= ceil(len/16): every
// loop below is static, so the compiler can batch the LDS reads ahead of the MFMAs); NT = NKT rounded up to even (k-steps of 32
// keys).  How keys >= len are masked is a compile-time policy -- the general form costs a compare-select pair on all 4 NKT scores:
// 150 of the ~650 VALU issues of a query tile, and this body is VALU-issue bound (54 MFMAs against ~600 VALU per tile):
//   MASK_EXACT  NKT == ceil(len/16): only the last key tile can hold keys >= len, only its 4 scores per lane carry mask code
//   MASK_ANY    every score is compared
//   MASK_LEN    len is only known at run time: the tiles from the last real one on carry mask code (a wave-uniform branch per
//               tile), and the last key counts `mult` times -- its probability is multiplied by wmul_last after the exponential
//               (exact for an integer in f32; the normaliser is the matrix-pipe sum of the same rounded values), or wadd_last
//               (log2(mult) / scale_log2e) is added to its score in front of the maximum.  The other two take no weight.
enum AttnMask { MASK_EXACT, MASK_ANY, MASK_LEN };

template <typename HT, int NKT, AttnMask MASK>
__device__ __forceinline__ void attn_fwd_body(char* smem, const HT* __restrict__ base, HT* __restrict__ obase,
                                              float* __restrict__ lse_row, int len, int H, float scale_log2e, float wmul_last,
                                              float wadd_last) {
  constexpr int NT = NKT + (NKT & 1);
  constexpr int nkt = NKT;
  char* Ks = smem;
  char* Vs = smem + nkt * 16 * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tok_stride = (int64_t)3 * H * ATT_D;  // elements between consecutive tokens
  // ---- stage K and V of this head.  Rows >= len duplicate row len - 1: their scores are masked and their probabilities are
  //      exactly 0, so they never contribute. ---------------------------------------------------------------------------------
  {
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    for (int pc = wave_u; pc < nkt * 2; pc += ATT_THREADS / 64) {
      stage_piece(Ks, pc, base + H * ATT_D + piece_off<false>(tok_stride, len, pc, lane));
      stage_piece(Vs, pc, base + 2 * H * ATT_D + piece_off<true>(tok_stride, len, pc, lane));
    }
  }
  const int g = lane >> 4, qi = lane & 15;
  const int nqt = (len + 15) >> 4;
  u32x4 qn0 = u32x4{0u, 0u, 0u, 0u}, qn1 = qn0;
  if (wave < nqt) load_q(base, tok_stride, len, wave, qi, g, qn0, qn1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // MASK_LEN: the weighted key is slot (g, r) of tile kt_last
  const int last = len - 1;
  const int kt_last = __builtin_amdgcn_readfirstlane(last >> 4);
  float wmul[4], wadd[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool is_last = (g * 4 + r) == (last & 15);
    wmul[r] = is_last ? wmul_last : 1.0f;
    wadd[r] = is_last ? wadd_last : 0.0f;
  }
  for (int qt = wave; qt < nqt; qt += ATT_THREADS / 64) {
    const int q0 = qt * 16;
    const u32x4 qf0 = qn0, qf1 = qn1;
    if (qt + ATT_THREADS / 64 < nqt) load_q(base, tok_stride, len, qt + ATT_THREADS / 64, qi, g, qn0, qn1);  // next tile's Q under this tile's math

    // ---- S^T tiles: fragment reads in batches of 4 key tiles (8 ds_read_b128) ahead of their 8 MFMAs; the
    //      sched_barrier keeps hipcc from either sinking each read next to its MFMA (one exposed LDS latency per
    //      MFMA) or hoisting all 26 reads (104 VGPRs, spills) --------------------------------------------------
    f32x4 sacc[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) sacc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int NKG = (nkt + 3) / 4;
    u32x4 kf[2][4][2];  // double-buffered: group gi+1 is read while group gi feeds the MFMAs
    auto read_k = [&](int buf, int kg) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (kg + i < nkt) {
          kf[buf][i][0] = *reinterpret_cast<const u32x4*>(Ks + img_off((kg + i) * 16 + qi, g));
          kf[buf][i][1] = *reinterpret_cast<const u32x4*>(Ks + img_off((kg + i) * 16 + qi, 4 + g));
        }
      }
    };
    read_k(0, 0);
#pragma unroll
    for (int gi = 0; gi < NKG; ++gi) {
      const int kg = gi * 4;
      if (gi + 1 < NKG) read_k((gi + 1) & 1, kg + 4);
      __builtin_amdgcn_sched_barrier(0);
      // first halves of the 4 tiles, then the second halves: the two MFMAs of one accumulator are 3 issues apart
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (kg + i < nkt) sacc[kg + i] = mma<HT>(kf[gi & 1][i][hf], hf ? qf1 : qf0, sacc[kg + i]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // keys >= len: -inf (their probability is exactly 0).  The odd padding tile NKT (when NT > NKT) has no scores at
    // all: it is left out of max / exp and stays zero into the packing below.
    if constexpr (MASK == MASK_EXACT) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if ((NKT - 1) * 16 + g * 4 + r >= len) sacc[NKT - 1][r] = -INFINITY;
    } else if constexpr (MASK == MASK_ANY) {
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kt * 16 + g * 4 + r >= len) sacc[kt][r] = -INFINITY;
    } else {
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        if (kt >= kt_last) {  // wave-uniform
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (kt == kt_last) sacc[kt][r] += wadd[r];  // the weighted key's score shift (0 unless the weight rides on the score)
            if (kt * 16 + g * 4 + r >= len) sacc[kt][r] = -INFINITY;
          }
        }
      }
    }
    float mm[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};  // four independent v_max3 chains, two per tile
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      mm[(2 * kt) & 3] = fmaxf(fmaxf(mm[(2 * kt) & 3], sacc[kt][0]), sacc[kt][1]);
      mm[(2 * kt + 1) & 3] = fmaxf(fmaxf(mm[(2 * kt + 1) & 3], sacc[kt][2]), sacc[kt][3]);
    }
    float m = fmaxf(fmaxf(mm[0], mm[1]), fmaxf(mm[2], mm[3]));
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float nmc = -m * scale_log2e;  // exp2(s*c - m*c): scale folded into one FMA per score
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sacc[kt][r] = __builtin_amdgcn_exp2f(fmaf(sacc[kt][r], scale_log2e, nmc));
      if constexpr (MASK == MASK_LEN) {
        if (kt == kt_last) {  // wave-uniform: the weighted key's probability counts mult times
#pragma unroll
          for (int r = 0; r < 4; ++r) sacc[kt][r] *= wmul[r];
        }
      }
    }

    // ---- O^T = V^T P^T: P packed to 16 bit first (frees the f32 scores), then per k-step 8 transposed reads issued
    //      together ahead of their 4 MFMAs --------------------------------------------------------------------------
    u32x4 pf[NT / 2];
#pragma unroll
    for (int ks = 0; ks < NT / 2; ++ks) pf[ks] = cvt8<HT>(sacc[2 * ks], sacc[2 * ks + 1]);
    f32x4 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // softmax denominator on the matrix pipe: an all-ones "V^T" fragment sums the (16-bit rounded) probabilities of
    // every query over the keys -- 7 MFMAs instead of 56 v_add + 2 cross-lane adds, and the normaliser is the sum
    // of exactly the values that multiply V
    f32x4 lacc = f32x4{0.f, 0.f, 0.f, 0.f};
    const int tq = qi >> 2, tp = qi & 3;  // transposed-read address roles inside the 16-lane group
    s16x4 v0[2][4], v1[2][4];  // double-buffered transposed V fragments
    auto read_v = [&](int buf, int ks) {
      const int row1 = 32 * ks + 4 * g + tq;  // row this lane addresses in block 1; block 2 is 16 rows further
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        v0[buf][dt] = s16x4{0, 0, 0, 0};
        v1[buf][dt] = s16x4{0, 0, 0, 0};
        if (2 * ks < nkt) v0[buf][dt] = tr_read(Vs + v_lds_off(row1, dt) + tp * 8);  // static
        // static: the padding tile has no rows in LDS (its P entries are zero anyway)
        if (2 * ks + 1 < nkt) v1[buf][dt] = tr_read(Vs + v_lds_off(row1 + 16, dt) + tp * 8);
      }
    };
    read_v(0, 0);
#pragma unroll
    for (int ks = 0; ks < NT / 2; ++ks) {
      if (ks + 1 < NT / 2) read_v((ks + 1) & 1, ks + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) oacc[dt] = mma<HT>(tr_join(v0[ks & 1][dt], v1[ks & 1][dt]), pf[ks], oacc[dt]);
      lacc = mma<HT>(ones<HT>(), pf[ks], lacc);
      __builtin_amdgcn_sched_barrier(0);
    }
    const float inv_l = 1.0f / lacc[0];
    // training: log2 of the softmax normaliser in the scaled-score domain, p = exp2(s c - lse) (the backward recomputes p from it)
    if (lse_row && g == 0 && q0 + qi < len) lse_row[q0 + qi] = fmaf(m, scale_log2e, __log2f(lacc[0]));
    if (q0 + qi < len) store_tile(obase + (int64_t)(q0 + qi) * (H * ATT_D) + g * 4, oacc, inv_l);
  }
}

}  // namespace
