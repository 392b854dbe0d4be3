// Skip-aware attention half for eval (models/resMoE.py:126-135 with a hard dense_gate): a bypassed token's operand row is exactly
// zero, so its q / k / v are the rounded qkv bias -- the same for every bypassed token.  Per image with n entering and m = N - n
// bypassed tokens the attention half therefore needs n + 1 rows (n when m == 0):
//   keys     the m identical bypassed keys are ONE key whose probability counts m times;
//   queries  the m identical bypassed queries are ONE query; its projection row c_b is added to every bypassed residual row.
// Three kernels:
//   smoe_skip_plan             mask -> per-image (row_start, len, mult), the compact gather list, the projection's row map, the
//                              one-group offsets [0, R] and every bypassed token's representative output row -- all on the device
//   smoe_attention_fwd_varlen  the one-pass forward (attention_tile.h) over the compact qkv, row range and key count per image from the
//                              plan, the last key of an image weighted by mult
//   smoe_skip_expand           out[t] = xn32[t] + out[rep_row[t]] for the bypassed tokens
// No allocation, no synchronisation, no float atomics; every output is a pure function of the inputs.
#include "attention_tile.h"

namespace {

constexpr int PLAN_THREADS = 256;

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
// attention_tile.h's attn_fwd_body with MASK_LEN: the rows of an (image, head) are base[0 .. len), key index >= len is masked at run
// time, the last key counts `mult` times (by default on its probability; SMOE_VARLEN_WEIGHT_SCORE: log2(mult) on its scaled score);
// no lse.
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
  if (NKTMAX > 4 && tiers && len <= 64) attn_fwd_body<HT, 4, MASK_LEN>(smem, base, obase, nullptr, len, H, scale_log2e, wmul, wadd);
  else if (NKTMAX > 8 && tiers && len <= 128) attn_fwd_body<HT, 8, MASK_LEN>(smem, base, obase, nullptr, len, H, scale_log2e, wmul, wadd);
  else if (NKTMAX > 13 && tiers && len <= 208) attn_fwd_body<HT, 13, MASK_LEN>(smem, base, obase, nullptr, len, H, scale_log2e, wmul, wadd);
  else attn_fwd_body<HT, NKTMAX, MASK_LEN>(smem, base, obase, nullptr, len, H, scale_log2e, wmul, wadd);
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
