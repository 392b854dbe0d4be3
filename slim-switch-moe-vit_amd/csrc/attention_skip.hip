// Skip-aware attention half for eval (models/resMoE.py:126-135 with a hard dense_gate): a bypassed token's operand row is exactly
// zero, so its q / k / v are the rounded qkv bias -- the same for every bypassed token.  Per image with n entering and m = N - n
// bypassed tokens the attention half therefore needs n + 1 rows (n when m == 0):
//   keys     the m identical bypassed keys are ONE key whose probability counts m times;
//   queries  the m identical bypassed queries are ONE query; its projection row c_b is added to every bypassed residual row.
// Three kernels:
//   smoe_skip_plan             mask -> per-image (row_start, len, mult), the compact gather list, the projection's row map, the
//                              one-group offsets [0, R] and every bypassed token's representative output row -- all on the device
//   smoe_attention_fwd_varlen  attention.hip's one-pass forward over the compact qkv, row range and key count per image from the
//                              plan, the last key of an image weighted by mult
//   smoe_skip_expand           out[t] = xn32[t] + out[rep_row[t]] for the bypassed tokens
// No allocation, no synchronisation, no float atomics; every output is a pure function of the inputs.
#include "smoe_common.h"
#include <type_traits>

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
constexpr int ATT_D = 64;
constexpr int ATT_THREADS = 256;
constexpr int PLAN_THREADS = 256;

// the LDS layouts of attention.hip (K: 16-byte chunk swizzle, V: 32-byte segment swizzle)
__device__ __forceinline__ int k_lds_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int v_lds_off(int row, int dt) { return row * 128 + ((dt ^ ((row >> 1) & 3)) << 5); }

// ---- plan ----------------------------------------------------------------------------------------------------------------------
// pass 1, one workgroup per image: len[b] = n_b + (m_b > 0), mult[b] = m_b; the parked output row of the image is zeroed (it is
// the projection's `residual` row of the representative)
__global__ __launch_bounds__(PLAN_THREADS) void skip_count_kernel(const float* __restrict__ mask, int N, int32_t* __restrict__ len,
                                                                 int32_t* __restrict__ mult, float* __restrict__ park, int park_cols) {
  __shared__ int wsum[PLAN_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* mk = mask + (int64_t)b * N * 2;
  int n = 0;
  for (int t = tid; t < N; t += PLAN_THREADS) n += mk[2 * t] > 0.5f ? 0 : 1;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) n += __shfl_xor(n, s, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < PLAN_THREADS / 64; ++w) tot += wsum[w];
    len[b] = tot + (tot < N ? 1 : 0);
    mult[b] = N - tot;
  }
  if (park)
    for (int c = tid; c < park_cols; c += PLAN_THREADS) park[(int64_t)b * park_cols + c] = 0.f;
}

// pass 2, one workgroup per image: row_start[b] = sum of len over the images before it; the entering tokens in token order, then
// the image's first bypassed token as the representative row.  The last image's workgroup also writes offsets and the unused tail.
__global__ __launch_bounds__(PLAN_THREADS) void skip_build_kernel(const float* __restrict__ mask, int B, int N,
                                                                  const int32_t* __restrict__ len, int32_t* __restrict__ row_start,
                                                                  int64_t* __restrict__ gather, int64_t* __restrict__ row_map,
                                                                  int32_t* __restrict__ offsets, int32_t* __restrict__ rep_row) {
  __shared__ int wsum[PLAN_THREADS / 64];
  __shared__ int first_bypass;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t T = (int64_t)B * N;
  int s = 0;
  for (int i = tid; i < b; i += PLAN_THREADS) s += len[i];
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k, 64);
  if (lane == 0) wsum[wave] = s;
  if (tid == 0) first_bypass = N;
  __syncthreads();
  int start = 0;
  for (int w = 0; w < PLAN_THREADS / 64; ++w) start += wsum[w];
  __syncthreads();
  const float* mk = mask + (int64_t)b * N * 2;
  int run = 0;  // entering tokens of this image before the current chunk
  for (int t0 = 0; t0 < N; t0 += PLAN_THREADS) {
    const int t = t0 + tid;
    const bool valid = t < N;
    const bool enter = valid && !(mk[2 * t] > 0.5f);
    const unsigned long long bal = __ballot(enter);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int wbase = 0, tot = 0;
    for (int w = 0; w < PLAN_THREADS / 64; ++w) {
      if (w < wave) wbase += wsum[w];
      tot += wsum[w];
    }
    if (enter) {
      const int64_t r = (int64_t)start + run + wbase + before;
      if (r < T) {  // (always: start + n_b <= b N + n_b)
        gather[r] = (int64_t)b * N + t;
        row_map[r] = (int64_t)b * N + t;
      }
      rep_row[(int64_t)b * N + t] = -1;
    } else if (valid) {
      rep_row[(int64_t)b * N + t] = (int32_t)(T + b);
      atomicMin(&first_bypass, t);
    }
    run += tot;
    __syncthreads();
  }
  if (tid == 0) {
    row_start[b] = start;
    int64_t R = (int64_t)start + run;
    if (run < N && R < T) {
      gather[R] = (int64_t)b * N + first_bypass;
      row_map[R] = T + b;
      ++R;
    }
    wsum[0] = (int)R;
    if (b == B - 1) { offsets[0] = 0; offsets[1] = (int32_t)R; }
  }
  if (b == B - 1) {
    __syncthreads();
    // rows at and past R belong to no group: a GEMM whose offsets end at R neither reads nor stores them; they hold valid indices
    for (int64_t r = (int64_t)wsum[0] + tid; r < T; r += PLAN_THREADS) { gather[r] = 0; row_map[r] = T; }
  }
}

// ---- expand --------------------------------------------------------------------------------------------------------------------
// one wave per token; only bypassed tokens (rep_row >= 0) are touched.  xn32 may be `out` itself (every element is read by the
// thread that writes it).
__global__ __launch_bounds__(256) void skip_expand_kernel(const float* xn32, const int32_t* __restrict__ rep_row, float* out,
                                                          int64_t T, int d, int64_t out_rows) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += nw) {
    const int rr = rep_row[t];
    if (rr < 0 || rr >= out_rows) continue;
    const f32x4* src = reinterpret_cast<const f32x4*>(xn32 + t * d);
    const f32x4* c = reinterpret_cast<const f32x4*>(out + (int64_t)rr * d);
    f32x4* dst = reinterpret_cast<f32x4*>(out + t * d);
    for (int i = lane; i < d / 4; i += 64) dst[i] = src[i] + c[i];
  }
}

// ---- varlen attention ------------------------------------------------------------------------------------------------------------
// attention.hip's attn_fwd_kernel for one (image, head) whose rows are base[0 .. len): NKT key tiles of 16 held in LDS (NKT * 16 >=
// len), key index >= len masked at run time -- only the tiles from the last real one on carry mask code (a wave-uniform branch per
// tile).  The last key counts `mult` times: its probability is multiplied by wmul after the exponential (exact for an integer in f32;
// the normaliser is the matrix-pipe sum of the same rounded values), or -- SMOE_VARLEN_WEIGHT_SCORE -- log2(mult) is added to its
// scaled score in front of the maximum.
template <typename HT, int NKT>
__device__ __forceinline__ void attn_varlen_body(char* smem, const HT* __restrict__ base, HT* __restrict__ obase, int len, int H,
                                                 float scale_log2e, float wmul_last, float wadd_last) {
  constexpr int NT = NKT + (NKT & 1);
  constexpr int nkt = NKT;
  char* Ks = smem;
  char* Vs = smem + nkt * 16 * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t tok_stride = (int64_t)3 * H * ATT_D;
  // stage K and V by LDS DMA; rows >= len duplicate row len - 1 (masked below: probability exactly 0)
  {
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int l_row = lane >> 3, l_pos = lane & 7;
    const int npieces = nkt * 2;
    for (int pc = wave_u; pc < npieces; pc += ATT_THREADS / 64) {
      const int row = pc * 8 + l_row;
      const int srow = row < len ? row : len - 1;
      const HT* p = base + (int64_t)srow * tok_stride;
      const int kc = l_pos ^ ((row >> 1) & 7);
      const int vc = (((l_pos >> 1) ^ ((row >> 1) & 3)) << 1) | (l_pos & 1);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p + H * ATT_D + kc * 8),
                                       (__attribute__((address_space(3))) void*)(Ks + pc * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p + 2 * H * ATT_D + vc * 8),
                                       (__attribute__((address_space(3))) void*)(Vs + pc * 1024), 16, 0, 0);
    }
  }
  const int g = lane >> 4, qi = lane & 15;
  const int nqt = (len + 15) >> 4;
  auto load_q = [&](int qt, u32x4& f0, u32x4& f1) {
    int qrow = qt * 16 + qi;
    if (qrow >= len) qrow = len - 1;
    const HT* qp = base + (int64_t)qrow * tok_stride + g * 8;
    f0 = *reinterpret_cast<const u32x4*>(qp);
    f1 = *reinterpret_cast<const u32x4*>(qp + 32);
  };
  u32x4 qn0 = u32x4{0u, 0u, 0u, 0u}, qn1 = qn0;
  if (wave < nqt) load_q(wave, qn0, qn1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // the weighted key: slot (g, r) of tile kt_last
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
    if (qt + ATT_THREADS / 64 < nqt) load_q(qt + ATT_THREADS / 64, qn0, qn1);
    f32x4 sacc[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) sacc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int NKG = (nkt + 3) / 4;
    u32x4 kf[2][4][2];
    auto read_k = [&](int buf, int kg) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (kg + i < nkt) {
          kf[buf][i][0] = *reinterpret_cast<const u32x4*>(Ks + k_lds_off((kg + i) * 16 + qi, g));
          kf[buf][i][1] = *reinterpret_cast<const u32x4*>(Ks + k_lds_off((kg + i) * 16 + qi, 4 + g));
        }
      }
    };
    read_k(0, 0);
#pragma unroll
    for (int gi = 0; gi < NKG; ++gi) {
      const int kg = gi * 4;
      if (gi + 1 < NKG) read_k((gi + 1) & 1, kg + 4);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (kg + i < nkt) {
            if constexpr (std::is_same<HT, f16>::value)
              sacc[kg + i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, kf[gi & 1][i][hf]), __builtin_bit_cast(f16x8, hf ? qf1 : qf0), sacc[kg + i], 0, 0, 0);
            else
              sacc[kg + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kf[gi & 1][i][hf]), __builtin_bit_cast(bf16x8_t, hf ? qf1 : qf0), sacc[kg + i], 0, 0, 0);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // keys >= len: -inf; the weighted key's score shift (0 unless the weight rides on the score)
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      if (kt >= kt_last) {  // wave-uniform
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (kt == kt_last) sacc[kt][r] += wadd[r];
          if (kt * 16 + g * 4 + r >= len) sacc[kt][r] = -INFINITY;
        }
      }
    }
    float mm[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      mm[(2 * kt) & 3] = fmaxf(fmaxf(mm[(2 * kt) & 3], sacc[kt][0]), sacc[kt][1]);
      mm[(2 * kt + 1) & 3] = fmaxf(fmaxf(mm[(2 * kt + 1) & 3], sacc[kt][2]), sacc[kt][3]);
    }
    float m = fmaxf(fmaxf(mm[0], mm[1]), fmaxf(mm[2], mm[3]));
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float nmc = -m * scale_log2e;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sacc[kt][r] = __builtin_amdgcn_exp2f(fmaf(sacc[kt][r], scale_log2e, nmc));
      if (kt == kt_last) {  // wave-uniform: the weighted key's probability counts mult times
#pragma unroll
        for (int r = 0; r < 4; ++r) sacc[kt][r] *= wmul[r];
      }
    }
    u32x4 pf[NT / 2];
#pragma unroll
    for (int ks = 0; ks < NT / 2; ++ks) {
      if constexpr (std::is_same<HT, f16>::value) {
        f16x8 t;
#pragma unroll
        for (int r = 0; r < 4; ++r) { t[r] = (f16)sacc[2 * ks][r]; t[4 + r] = (2 * ks + 1 < NKT) ? (f16)sacc[2 * ks + 1][r] : (f16)0.f; }
        pf[ks] = __builtin_bit_cast(u32x4, t);
      } else {
        s16x8 t;
#pragma unroll
        for (int r = 0; r < 4; ++r) { t[r] = (short)f32_to_bf16(sacc[2 * ks][r]); t[4 + r] = (2 * ks + 1 < NKT) ? (short)f32_to_bf16(sacc[2 * ks + 1][r]) : (short)0; }
        pf[ks] = __builtin_bit_cast(u32x4, t);
      }
    }
    f32x4 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 lacc = f32x4{0.f, 0.f, 0.f, 0.f};
    const u32x4 ones = std::is_same<HT, f16>::value ? u32x4{0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u}
                                                    : u32x4{0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
    const int tq = qi >> 2, tp = qi & 3;
    s16x4 v0[2][4], v1[2][4];
    auto read_v = [&](int buf, int ks) {
      const int row1 = 32 * ks + 4 * g + tq;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        v0[buf][dt] = s16x4{0, 0, 0, 0};
        v1[buf][dt] = s16x4{0, 0, 0, 0};
        if (2 * ks < nkt)
          v0[buf][dt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(Vs + v_lds_off(row1, dt) + tp * 8));
        if (2 * ks + 1 < nkt)
          v1[buf][dt] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(Vs + v_lds_off(row1 + 16, dt) + tp * 8));
      }
    };
    read_v(0, 0);
#pragma unroll
    for (int ks = 0; ks < NT / 2; ++ks) {
      if (ks + 1 < NT / 2) read_v((ks + 1) & 1, ks + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        s16x8 vf;
#pragma unroll
        for (int r = 0; r < 4; ++r) { vf[r] = v0[ks & 1][dt][r]; vf[4 + r] = v1[ks & 1][dt][r]; }
        if constexpr (std::is_same<HT, f16>::value)
          oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, vf), __builtin_bit_cast(f16x8, pf[ks]), oacc[dt], 0, 0, 0);
        else
          oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, vf), __builtin_bit_cast(bf16x8_t, pf[ks]), oacc[dt], 0, 0, 0);
      }
      if constexpr (std::is_same<HT, f16>::value)
        lacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, ones), __builtin_bit_cast(f16x8, pf[ks]), lacc, 0, 0, 0);
      else
        lacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ones), __builtin_bit_cast(bf16x8_t, pf[ks]), lacc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    const float inv_l = 1.0f / lacc[0];
    if (q0 + qi < len) {
      HT* op = obase + (int64_t)(q0 + qi) * (H * ATT_D) + g * 4;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        if constexpr (std::is_same<HT, f16>::value) {
          f16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (f16)(oacc[dt][r] * inv_l);
          *reinterpret_cast<f16x4*>(op + dt * 16) = o;
        } else {
          s16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (short)f32_to_bf16(oacc[dt][r] * inv_l);
          *reinterpret_cast<s16x4*>(op + dt * 16) = o;
        }
      }
    }
  }
}

// One workgroup per (image, head).  NKTMAX covers the caller's max_len; with tiers an image takes the smallest instantiated key-tile
// count that holds its own len (a workgroup-uniform choice: same launch, fewer score registers walked for short images).
template <typename HT, int NKTMAX>
__global__ __launch_bounds__(ATT_THREADS, 3) void attn_varlen_kernel(const HT* __restrict__ qkv, HT* __restrict__ out,
                                                                     const int32_t* __restrict__ row_start,
                                                                     const int32_t* __restrict__ len_p,
                                                                     const int32_t* __restrict__ mult_p, int64_t rows_cap, int H,
                                                                     float scale_log2e, int flags) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int rs = __builtin_amdgcn_readfirstlane(row_start[b]);
  const int len = __builtin_amdgcn_readfirstlane(len_p[b]);
  const int mult = __builtin_amdgcn_readfirstlane(mult_p[b]);
  // a plan that does not fit the buffers or this instantiation is not followed (no wild access; the rows stay unwritten)
  if (len < 1 || len > NKTMAX * 16 || rs < 0 || (int64_t)rs + len > rows_cap || mult < 0) return;
  const HT* base = qkv + (int64_t)rs * 3 * H * ATT_D + h * ATT_D;
  HT* obase = out + (int64_t)rs * H * ATT_D + h * ATT_D;
  float wmul = 1.0f, wadd = 0.0f;
  if (mult > 0) {
    if (flags & SMOE_VARLEN_WEIGHT_SCORE) wadd = __log2f((float)mult) / scale_log2e;
    else wmul = (float)mult;
  }
  const bool tiers = !(flags & SMOE_VARLEN_NO_TIERS);
  if (NKTMAX > 4 && tiers && len <= 64) attn_varlen_body<HT, 4>(smem, base, obase, len, H, scale_log2e, wmul, wadd);
  else if (NKTMAX > 8 && tiers && len <= 128) attn_varlen_body<HT, 8>(smem, base, obase, len, H, scale_log2e, wmul, wadd);
  else if (NKTMAX > 13 && tiers && len <= 208) attn_varlen_body<HT, 13>(smem, base, obase, len, H, scale_log2e, wmul, wadd);
  else attn_varlen_body<HT, NKTMAX>(smem, base, obase, len, H, scale_log2e, wmul, wadd);
}

template <typename HT, int NKTMAX>
int launch_varlen(const void* qkv, void* out, const int32_t* row_start, const int32_t* len, const int32_t* mult, int B,
                  int64_t rows_cap, int H, float scale, int flags, hipStream_t s) {
  const size_t smem = 2 * (size_t)NKTMAX * 16 * 128;
  SMOE_ENSURE_SMEM(attn_varlen_kernel<HT, NKTMAX>);
  hipLaunchKernelGGL((attn_varlen_kernel<HT, NKTMAX>), dim3(B * H), dim3(ATT_THREADS), smem, s, (const HT*)qkv, (HT*)out, row_start,
                     len, mult, rows_cap, H, scale * 1.4426950408889634f, flags);
  SMOE_CHECK_LAUNCH("smoe_attention_fwd_varlen");
  return 0;
}

template <typename HT>
int varlen_dispatch(const void* qkv, void* out, const int32_t* row_start, const int32_t* len, const int32_t* mult, int B,
                    int max_len, int64_t rows_cap, int H, float scale, int flags, hipStream_t s) {
  if (max_len <= 64) return launch_varlen<HT, 4>(qkv, out, row_start, len, mult, B, rows_cap, H, scale, flags, s);
  if (max_len <= 128) return launch_varlen<HT, 8>(qkv, out, row_start, len, mult, B, rows_cap, H, scale, flags, s);
  if (max_len <= 208) return launch_varlen<HT, 13>(qkv, out, row_start, len, mult, B, rows_cap, H, scale, flags, s);
  return launch_varlen<HT, 16>(qkv, out, row_start, len, mult, B, rows_cap, H, scale, flags, s);
}

}  // namespace

extern "C" int smoe_skip_plan(const float* mask, int B, int N, int32_t* row_start, int32_t* len, int32_t* mult, int64_t* gather,
                              int64_t* row_map, int32_t* offsets, int32_t* rep_row, float* park, int park_cols, void* stream) {
  SMOE_REQUIRE(B >= 0 && N >= 1 && (int64_t)B * N + B < ((int64_t)1 << 31), "smoe_skip_plan: bad B=%d N=%d (B N + B < 2^31)", B, N);
  SMOE_REQUIRE(park_cols >= 0, "smoe_skip_plan: bad park_cols=%d", park_cols);
  if (B == 0) return 0;
  SMOE_REQUIRE(mask && row_start && len && mult && gather && row_map && offsets && rep_row, "smoe_skip_plan: null pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(skip_count_kernel, dim3(B), dim3(PLAN_THREADS), 0, s, mask, N, len, mult, park, park_cols);
  SMOE_CHECK_LAUNCH("smoe_skip_plan/count");
  hipLaunchKernelGGL(skip_build_kernel, dim3(B), dim3(PLAN_THREADS), 0, s, mask, B, N, len, row_start, gather, row_map, offsets,
                     rep_row);
  SMOE_CHECK_LAUNCH("smoe_skip_plan/build");
  return 0;
}

extern "C" int smoe_attention_fwd_varlen(const void* qkv, void* out, int dtype, const int32_t* row_start, const int32_t* len,
                                         const int32_t* mult, int B, int max_len, int64_t rows_cap, int H, int head_dim, float scale,
                                         int flags, void* stream) {
  SMOE_REQUIRE(max_len >= 1 && max_len <= 256 && head_dim == ATT_D, "smoe_attention_fwd_varlen: unsupported max_len=%d head_dim=%d "
               "(max_len <= 256, head_dim 64)", max_len, head_dim);
  SMOE_REQUIRE(B >= 0 && H >= 1 && rows_cap >= 0, "smoe_attention_fwd_varlen: bad B=%d H=%d rows_cap=%lld", B, H, (long long)rows_cap);
  SMOE_REQUIRE(!(flags & ~(SMOE_VARLEN_WEIGHT_SCORE | SMOE_VARLEN_NO_TIERS)), "smoe_attention_fwd_varlen: unknown flags %d", flags);
  if (B == 0) return 0;
  SMOE_REQUIRE(qkv && out && row_start && len && mult, "smoe_attention_fwd_varlen: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SMOE_F16) return varlen_dispatch<f16>(qkv, out, row_start, len, mult, B, max_len, rows_cap, H, scale, flags, s);
  if (dtype == SMOE_BF16) return varlen_dispatch<bf16_bits>(qkv, out, row_start, len, mult, B, max_len, rows_cap, H, scale, flags, s);
  smoe_set_error("smoe_attention_fwd_varlen: dtype must be f16 or bf16");
  return 1;
}

extern "C" int smoe_skip_expand(const float* xn32, const int32_t* rep_row, float* out, int64_t T, int d, int64_t out_rows,
                                void* stream) {
  SMOE_REQUIRE(T >= 0 && d >= 4 && d % 4 == 0 && out_rows >= T, "smoe_skip_expand: bad T=%lld d=%d out_rows=%lld (d %% 4 == 0)",
               (long long)T, d, (long long)out_rows);
  if (T == 0) return 0;
  SMOE_REQUIRE(xn32 && rep_row && out, "smoe_skip_expand: null pointer");
  const int64_t blocks = (T + 3) / 4;
  hipLaunchKernelGGL(skip_expand_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, xn32,
                     rep_row, out, T, d, out_rows);
  SMOE_CHECK_LAUNCH("smoe_skip_expand");
  return 0;
}
