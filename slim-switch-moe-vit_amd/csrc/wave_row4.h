// The 4-wide wave-per-row layout of the LayerNorm family: ONE WAVE holds one row of d <= 1024 floats (d % 4 == 0), lane l holds the
// 4-float chunks l + 64 j, j < NJ = ceil(d / 256), as v[j][0..4) (zeros at and past nchunk = d / 4).  What the kernels of this layout
// share is written here once -- layernorm_bwd_kernel / gate_ln_bwd_kernel (dense_bwd.hip), soft_gate_ln_fwd_kernel (soft_gate.hip),
// switch_ln_fwd_kernel / switch_ln_bwd_dx_kernel (switch_ln.hip) -- so that "the same arithmetic" between two of them is the same
// code: the soft gate's forward statistics are the ones gate_ln_bwd_kernel recomputes, gate_ln_bwd_kernel with its gate off is
// layernorm_bwd_kernel (tests/test_gpu_dense.py).  The library is built with -ffp-contract=on: an expression's shape here IS its
// rounding (the first pass pairs (a + b) + (c + d)).
// Which kernel takes which piece was settled by its registers (profiles/wave_row4_isa.txt): a piece that cost a kernel VGPRs stayed in
// that kernel -- the per-lane gamma / beta / w loads and the dx tail everywhere, the row loads of gate_ln_bwd_kernel (three tensors, one
// optional) and of the two SwitchableLayerNorm kernels.
// The 8-floats-per-lane layout of the forward LayerNorms is wave_row_stats / wave_row_affine in smoe_common.h.
#pragma once
#include "smoe_common.h"
#include <type_traits>

// ---- the row ----------------------------------------------------------------------------------------------------------------------
// wr4_load(nchunk, lane, wr4_row(x_row, xv), wr4_row(dy_row, gv), ...): the rows of several tensors (any load4 dtype) into v[NJ][4]
// under ONE bounds test per chunk
template <typename XT, int NJ> struct Wr4Row { const XT* row; float (&v)[NJ][4]; };
template <typename XT, int NJ> __device__ __forceinline__ Wr4Row<XT, NJ> wr4_row(const XT* row, float (&v)[NJ][4]) { return {row, v}; }
template <int NJ, typename... XT> __device__ __forceinline__ void wr4_load(int nchunk, int lane, Wr4Row<XT, NJ>... r) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < nchunk) (load4(r.row + c * 4, r.v[j]), ...);
    else ((r.v[j][0] = r.v[j][1] = r.v[j][2] = r.v[j][3] = 0.f), ...);
  }
}

// ---- statistics -------------------------------------------------------------------------------------------------------------------
// Two passes in registers: mean, rstd = rsqrt(biased var + eps).  PIVOT: about the row's first element -- xv BECOMES x - pivot (exact,
// or rounded at the size of the row's spread), mean = mean(x - pivot), and the pivot is returned (0 without PIVOT, xv untouched).  A
// common offset of the row (x = 300 + noise) then costs the mean nothing: an f32 sum of the raw values would carry the offset's
// rounding (ulp(300 d) / d per row) into every x - mean.
template <bool PIVOT, int NJ>
__device__ __forceinline__ float wr4_row_stats(float (&xv)[NJ][4], int nchunk, int lane, float inv_d, float eps, float& mean,
                                               float& rstd) {
  float pivot = 0.f;
  if constexpr (PIVOT) pivot = __shfl(xv[0][0], 0, 64);
  float s1 = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if constexpr (PIVOT) {
      const bool in = lane + 64 * j < nchunk;
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[j][i] = in ? xv[j][i] - pivot : 0.f;
    }
    s1 += (xv[j][0] + xv[j][1]) + (xv[j][2] + xv[j][3]);
  }
  mean = wave_sum(s1) * inv_d;
  float s2 = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (lane + 64 * j < nchunk) {
#pragma unroll
      for (int i = 0; i < 4; ++i) { const float dv = xv[j][i] - mean; s2 = fmaf(dv, dv, s2); }
    }
  }
  rstd = rsqrtf(wave_sum(s2) * inv_d + eps);
  return pivot;
}

// What follows the statistics stays in each kernel's own loops, in one form: xhat = in ? (x - mean) * rstd : 0.f (a product of its
// own), xn = in ? fmaf(xhat, gamma, beta) : 0.f, g = the gradient of the normed row times gamma, the per-lane sums c1 += g and
// c2 = fmaf(g, xhat, c2) beside the kernel's other accumulations, c = wave_sum(c) * inv_d, dx = rstd * (g - c1 - xhat * c2) [+ dres].
// As helpers -- a pass over the row, one element, or the whole dx tail -- they changed the kernels' registers
// (switch_ln_bwd_dx_kernel: 6 - 9 more VGPRs from a one-element xhat helper alone; profiles/wave_row4_ab.md).

// ---- deterministic column sums ------------------------------------------------------------------------------------------------------
// Every wave kept N per-lane accumulator rows acc[n][j][i] over the rows it walked; the WAVES waves of the workgroup meet in LDS in wave
// order and the workgroup writes ONE partial row [N][d] to out_row (no atomics; wr4_reduce_partials adds the partial rows in workgroup
// order).  All threads of the workgroup call it; its barrier also publishes whatever the caller wrote to LDS before the call.
template <int N, int NJ, int WAVES>
__device__ __forceinline__ void wr4_flush_cols(float (&red)[WAVES][N][NJ * 256], const float (&acc)[N][NJ][4], int d,
                                               float* out_row) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int n = 0; n < N; ++n) red[wave][n][(lane + 64 * j) * 4 + i] = acc[n][j][i];
  __syncthreads();
  for (int c = tid; c < N * d; c += WAVES * 64) {
    int n = 0, col = c;
#pragma unroll
    for (int k = 1; k < N; ++k)
      if (col >= d) { col -= d; ++n; }
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += red[w][n][col];
    out_row[c] = s;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// workgroups of a row-strided launch: one row per wave, `waves` per workgroup, at most per_cu workgroups per CU
inline int wr4_grid(int64_t T, int waves, int per_cu) {
  int64_t need = (T + waves - 1) / waves;
  const int64_t cap = (int64_t)smoe_num_cus() * per_cu;
  if (need > cap) need = cap;
  return (int)(need < 1 ? 1 : need);
}

// f(std::integral_constant<int, NJ>) for nj = (d / 4 + 63) / 64 chunks per lane; false (f not called) outside 1 .. 4, i.e. past
// d = 1024.  The entry points keep their own rejection of the widths they do not take.
template <typename F> inline bool wr4_dispatch_nj(int nj, F&& f) {
  switch (nj) {
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 3: f(std::integral_constant<int, 3>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    default: return false;
  }
}

// out[c] (c < L) = sum over the n_rows partial rows [n_rows][L] at `partial`, in row order, in two launches on s: WR4_STAGE1 row
// groups into the [WR4_STAGE1][L] floats that lie BEHIND the partial rows, then one.  Columns from `split` on go to out_b[c - split]
// (split = L: everything to out_a).  Defined once, in dense_bwd.hip.
constexpr int WR4_STAGE1 = 16;
void wr4_reduce_partials(float* partial, int n_rows, int L, float* out_a, int split, float* out_b, hipStream_t s);
