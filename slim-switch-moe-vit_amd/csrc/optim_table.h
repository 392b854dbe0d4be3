// The table toolkit of the optimizer-side kernels (optim.hip: gradient norm, AdamW, weight EMA; lamb.hip: LAMB's two stages).
//
// A multi-tensor launch covers every tensor of a step with one grid.  Its tables (built by optim.py, small host-to-device copies):
//   tab = int64 [rows][n_t] : rows of addresses, the LAST row the element counts (AdamW / LAMB / norm pass: p, g, exp_avg, exp_avg_sq, n;
//                             EMA: ema, model, n)
//   blk = int32 [2][n_blocks]: tensor of workgroup b, OPT_BLOCK-element block inside that tensor
// One workgroup of OPT_THREADS threads owns one block; thread x takes elements base + 4 x, + 4 x + 4 OPT_THREADS, ... as 16-byte
// vectors, the tensor's last 1 - 3 elements one by one.  What is here is what those kernels share; profiles/optim_table_ab.md has
// what each of them takes, at which registers.
#pragma once
#include "smoe_common.h"
#include <type_traits>

constexpr int OPT_THREADS = 256;
constexpr int OPT_BLOCK = 16384;   // elements per workgroup of every multi-tensor kernel (optim.py: SUMSQ_BLOCK)

// one gradient element as float (the scalar tails; the vector bodies use load4 / load8)
template <typename GT>
__device__ __forceinline__ float grad_at(const GT* __restrict__ g, int64_t j) {
  if constexpr (std::is_same<GT, float>::value) return g[j];
  else if constexpr (std::is_same<GT, f16>::value) return (float)g[j];
  else return bf16_to_f32(g[j]);
}

// the 16-bit image of a parameter (the MFMA operand copy the forward reads): elements [i, i + 4) / element j; no image: nothing
__device__ __forceinline__ void image_store4(void* sh, int sh_dtype, int64_t i, const f32x4& pv) {
  if (!sh) return;
  if (sh_dtype == SMOE_F16) {
    f16x4 h; h[0] = (f16)pv[0]; h[1] = (f16)pv[1]; h[2] = (f16)pv[2]; h[3] = (f16)pv[3];
    *reinterpret_cast<f16x4*>(reinterpret_cast<f16*>(sh) + i) = h;
  } else {
    s16x4 h; h[0] = (short)f32_to_bf16(pv[0]); h[1] = (short)f32_to_bf16(pv[1]); h[2] = (short)f32_to_bf16(pv[2]); h[3] = (short)f32_to_bf16(pv[3]);
    *reinterpret_cast<s16x4*>(reinterpret_cast<bf16_bits*>(sh) + i) = h;
  }
}
__device__ __forceinline__ void image_store1(void* sh, int sh_dtype, int64_t j, float p) {
  if (!sh) return;
  if (sh_dtype == SMOE_F16) reinterpret_cast<f16*>(sh)[j] = (f16)p;
  else reinterpret_cast<bf16_bits*>(sh)[j] = f32_to_bf16(p);
}

// ---- this workgroup's (tensor, block) of a multi-tensor launch ----------------------------------------------------------------
// The table is caller data: false for a tensor index outside [0, n_t), and the kernel returns.
__device__ __forceinline__ bool opt_tensor(const int32_t* __restrict__ blk, int n_t, int& t) {
  t = blk[blockIdx.x];
  return t >= 0 && t < n_t;
}
// row ROW of tab for tensor t: an address (as T*) or, in the last row, the element count
template <int ROW>
__device__ __forceinline__ int64_t opt_entry(const int64_t* __restrict__ tab, int n_t, int t) { return tab[(int64_t)ROW * n_t + t]; }
template <typename T, int ROW>
__device__ __forceinline__ T* opt_row(const int64_t* __restrict__ tab, int n_t, int t) {
  return reinterpret_cast<T*>(opt_entry<ROW>(tab, n_t, t));
}
// first element of this workgroup's block, and one past its last (n = the tensor's element count)
__device__ __forceinline__ int64_t opt_base(const int32_t* __restrict__ blk, int64_t n_blocks) {
  return (int64_t)blk[n_blocks + blockIdx.x] * OPT_BLOCK;
}
__device__ __forceinline__ int64_t opt_end(int64_t base, int64_t n) { return base + OPT_BLOCK < n ? base + OPT_BLOCK : n; }
// shadow = int64 [2][n_t] (optional): address and dtype code of every tensor's 16-bit image (0: none)
__device__ __forceinline__ void* opt_image(const int64_t* __restrict__ shadow, int t) { return shadow ? reinterpret_cast<void*>(shadow[t]) : nullptr; }
__device__ __forceinline__ int opt_image_dtype(const int64_t* __restrict__ shadow, int n_t, int t) {
  return shadow ? (int)shadow[(int64_t)n_t + t] : SMOE_F16;
}

// ---- the workgroup's sum: thread, wave (wave_sum), then the four waves in the fixed order (w0 + w1) + (w2 + w3) ---------------------
// Thread 0 stores the result.  The pair form sums two values under ONE barrier (red: OPT_THREADS / 64 floats per value).
__device__ __forceinline__ void wg_sum_to(float a, float* __restrict__ red, float* __restrict__ out) {
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ void wg_sum2_to(float a, float b, float (*__restrict__ red)[OPT_THREADS / 64], float* __restrict__ out_a,
                                           float* __restrict__ out_b) {
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    *out_a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    *out_b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// launch(tag) with tag = TagF32 / TagF16 / TagBF16 for the gradient dtype code (checked by the caller): the launch is written once,
//   opt_dispatch_grad(g_dtype, [&](auto tag) { using GT = typename decltype(tag)::T; hipLaunchKernelGGL(kernel<GT>, ...); });
template <typename Launch>
static inline void opt_dispatch_grad(int g_dtype, Launch&& launch) {
  switch (g_dtype) {
    case SMOE_F32: launch(TagF32{}); break;
    case SMOE_F16: launch(TagF16{}); break;
    default: launch(TagBF16{}); break;
  }
}

// what every _multi entry point requires of its counts (the grid is n_blocks) and, where it has one, of its gradient dtype
static inline bool opt_multi_ok(int n_tensors, int64_t n_blocks, int g_dtype = SMOE_F32) {
  return n_tensors >= 0 && n_blocks >= 0 && n_blocks < (1ll << 31) && smoe_dtype_ok(g_dtype);
}
