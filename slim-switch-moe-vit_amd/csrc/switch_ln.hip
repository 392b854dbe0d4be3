// SwitchableLayerNorm (models/layers.py:31-157; the rule of its forward, 105-151) -- the `router` of SwitchableVisionTransformer
// (models/vision_transformer.py:407, 591).  Per row of x [T, d] f32:
//     mean, biased var over d;  xhat = (x - mean) rsqrt(var + eps);
//     bucket b = the given one, or argmin_k sum_j (x_j - c_kj)^2 over the RAW row (first minimum; a NaN distance counts as the
//                smallest and the first NaN wins: torch.argmin);
//     y = xhat weights[b] + biases[b].
// Forward: ONE launch, one wave per row (a row of d <= 1024 floats = up to 16 per lane: the layout of wave_row4.h), the
// statistics two-pass in registers.  The K distances are accumulated in DOUBLE in the direct form: upstream's f32 expanded form
// |x|^2 + |c|^2 - 2 x.c misassigns rows near a bisector, the f64 direct form is the float64 evaluation itself up to summation order
// (relative error ~ d 2^-53).  K d f64 FMAs per row on a full-rate f64 pipe.  The centroids are always staged in LDS: up to 48 KB
// with four waves per workgroup and several workgroups per CU, above that (to 128 KB) with one 16-wave workgroup per CU.
// The K per-lane sums meet across the wave by halving (K - 1 + 6 - log2 K double shuffles instead of 6 K), in a fixed order.
// Backward: dx in the form wave_row4.h states (statistics recomputed from x, gamma = weights[b] per row) in one launch that also
// leaves the row statistics; the per-bucket sums dweights[k] = sum_{rows of k} dy xhat, dbiases[k] = sum dy in a second launch where a
// thread owns a COLUMN and walks rows -- its K x 2 accumulators live in LDS (a register array indexed by the bucket would go to
// scratch), every workgroup writes one partial table, two reduce launches add them in workgroup order: no atomics, the same bits
// run to run, and the rows of an empty bucket are sums of nothing = exact zeros.
#include "wave_row4.h"
#include <math.h>

namespace {

constexpr int SLN_THREADS = 256;
constexpr int SLN_WAVES = SLN_THREADS / 64;
constexpr int SLN_BIG_THREADS = 1024;     // the forward's workgroup when the centroid table leaves room for one workgroup per CU
constexpr int SLN_LDS_FLOATS = 12288;      // a centroid table of up to K * d = this (48 KB) runs SLN_THREADS-wide workgroups, several per CU
constexpr int SLN_MAX_K = 32;

// torch.argmin's order on (distance, index): a NaN beats every number, among equals (or two NaNs) the smaller index wins
__device__ __forceinline__ bool sln_better(double a, int ka, double b, int kb) {
  const bool na = a != a, nb = b != b;
  if (na || nb) return na && (!nb || ka < kb);
  return a < b || (a == b && ka < kb);
}

template <int KP> struct SlnLog2 { static constexpr int v = 1 + SlnLog2<KP / 2>::v; };
template <> struct SlnLog2<1> { static constexpr int v = 0; };

// a[k] = this lane's share of distance k (k < KP, KP a power of two >= 2).  Returns the argmin over k < KP, the same in every lane.
// Stage s (mask m = 32 >> s) halves the values a lane holds: a lane whose bit m is set keeps the odd ones and sends the even ones to
// its partner.  After log2 KP stages a lane holds one value: bucket k(lane), bit s of k = bit (5 - s) of the lane.
template <int KP>
__device__ __forceinline__ int sln_argmin(double (&a)[KP], int lane) {
  constexpr int LG = SlnLog2<KP>::v;
  int k = 0;
#pragma unroll
  for (int s = 0; s < LG; ++s) {
    const int m = 32 >> s;
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < (KP >> (s + 1)); ++i) {
      const double send = up ? a[2 * i] : a[2 * i + 1];
      const double keep = up ? a[2 * i + 1] : a[2 * i];
      a[i] = keep + __shfl_xor(send, m, 64);
    }
    k |= (up ? 1 : 0) << s;
  }
  double v = a[0];
#pragma unroll
  for (int m = 32 >> LG; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
#pragma unroll
  for (int s = 0; s < LG; ++s) {
    const int m = 32 >> s;
    const double ov = __shfl_xor(v, m, 64);
    const int ok = __shfl_xor(k, m, 64);
    if (sln_better(ov, ok, v, k)) { v = ov; k = ok; }
  }
  return k;
}

// KP = 0: the bucket is given (buckets_in, or bucket_all for every row); KP >= 2: selected among K <= KP centroids.
// The centroids lie in dynamic LDS, staged once per workgroup: K d x 4 bytes.  THREADS = SLN_THREADS up to SLN_LDS_FLOATS (several
// workgroups per CU); a larger table (up to 128 KB of the CU's 160) leaves room for ONE workgroup per CU, which then has THREADS =
// SLN_BIG_THREADS = 16 waves to keep four waves per SIMD.  (Read from global memory instead, the table came back from L2 for every
// row and the hoisted loads took 256 VGPRs: 940 us at T = 50k, d = 768, K = 32 -- profiles/r22_switch_ln.md.)
template <int NJ, int KP, int THREADS>
__global__ __launch_bounds__(THREADS) void switch_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ weights,
                                                                    const float* __restrict__ biases,
                                                                    const float* __restrict__ centroids,
                                                                    const int64_t* __restrict__ buckets_in, int bucket_all, float eps,
                                                                    int64_t T, int d, int K, float* __restrict__ y,
                                                                    int64_t* __restrict__ buckets_out) {
  extern __shared__ float sln_cent[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = d >> 2;
  if (KP > 0) {
    const int n4 = (K * d) >> 2;
    for (int i = tid; i < n4; i += THREADS)
      reinterpret_cast<f32x4*>(sln_cent)[i] = reinterpret_cast<const f32x4*>(centroids)[i];
    __syncthreads();
  }
  const float inv_d = 1.0f / (float)d;
  const float qnan = __uint_as_float(0x7fc00000u);
  const int64_t row0 = (int64_t)blockIdx.x * (THREADS / 64) + wave, stride = (int64_t)gridDim.x * (THREADS / 64);
  for (int64_t t = row0; t < T; t += stride) {
    float xv[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {     // (its own row load: through wr4_load the kernel took 2 - 4 more VGPRs)
      const int c = lane + 64 * j;
      if (c < nchunk) {
        load4(x + t * (int64_t)d + c * 4, xv[j]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[j][i] = 0.f;
      }
    }
    int64_t b;
    if constexpr (KP > 0) {
      double a[KP];
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        if (k < K) {
          double s = 0.0;
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int c = lane + 64 * j;
            if (c < nchunk) {
              const f32x4 cv = *reinterpret_cast<const f32x4*>(sln_cent + k * d + c * 4);
#pragma unroll
              for (int i = 0; i < 4; ++i) { const double dv = (double)xv[j][i] - (double)cv[i]; s = fma(dv, dv, s); }
            }
          }
          a[k] = s;
        } else {
          a[k] = (double)INFINITY;     // a padded slot never wins: bucket 0 is real and ties go to the smaller index
        }
      }
      b = sln_argmin<KP>(a, lane);
    } else {
      b = buckets_in ? buckets_in[t] : (int64_t)bucket_all;
    }
    const bool in_range = b >= 0 && b < (int64_t)K;
    float mean, rstd;
    wr4_row_stats<true, NJ>(xv, nchunk, lane, inv_d, eps, mean, rstd);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      if (c < nchunk) {
        f32x4 o;
        if (!in_range) {
          o = f32x4{qnan, qnan, qnan, qnan};     // a bucket outside [0, K): nothing is read from the tables, the row is NaN
        } else if (weights) {
          const f32x4 g = *reinterpret_cast<const f32x4*>(weights + b * (int64_t)d + c * 4);
          const f32x4 be = biases ? *reinterpret_cast<const f32x4*>(biases + b * (int64_t)d + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = fmaf((xv[j][i] - mean) * rstd, g[i], be[i]);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = (xv[j][i] - mean) * rstd;
        }
        *reinterpret_cast<f32x4*>(y + t * (int64_t)d + c * 4) = o;
      }
    }
    if (lane == 0) buckets_out[t] = b;
  }
}

// dx[t] = rstd (g - mean(g) - xhat mean(g xhat)),  g = dy weights[b_t]  (weights null: g = dy);  stats[t] = (pivot, mean - pivot, rstd, -): the row statistics of wr4_row_stats<true>.
// A bucket outside [0, K) reads nothing from the table and gives a NaN row.
template <typename DYT, int NJ>
__global__ __launch_bounds__(SLN_THREADS) void switch_ln_bwd_dx_kernel(const float* __restrict__ x, const DYT* __restrict__ dy,
                                                                       const float* __restrict__ weights,
                                                                       const int64_t* __restrict__ buckets, float eps, int64_t T,
                                                                       int d, int K, float* __restrict__ dx,
                                                                       float* __restrict__ stats) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = d >> 2;
  const float inv_d = 1.0f / (float)d;
  const float qnan = __uint_as_float(0x7fc00000u);
  const int64_t row0 = (int64_t)blockIdx.x * SLN_WAVES + wave, stride = (int64_t)gridDim.x * SLN_WAVES;
  for (int64_t t = row0; t < T; t += stride) {
    const int64_t b = buckets[t];
    const bool in_range = b >= 0 && b < (int64_t)K;
    float xv[NJ][4], gv[NJ][4];
    // its own row load: g = dy weights[b] under the chunk's one bounds test (behind wr4_load the product lives twice across the
    // multiply's branch: 12 - 16 more VGPRs; profiles/wave_row4_ab.md)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      if (c < nchunk) {
        load4(x + t * (int64_t)d + c * 4, xv[j]);
        load4(dy + t * (int64_t)d + c * 4, gv[j]);
        if (weights && in_range) {
          const f32x4 g = *reinterpret_cast<const f32x4*>(weights + b * (int64_t)d + c * 4);
#pragma unroll
          for (int i = 0; i < 4; ++i) gv[j][i] *= g[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[j][i] = gv[j][i] = 0.f;
      }
    }
    float mean, rstd;
    const float pivot = wr4_row_stats<true, NJ>(xv, nchunk, lane, inv_d, eps, mean, rstd);
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float xh = (lane + 64 * j < nchunk) ? (xv[j][i] - mean) * rstd : 0.f;
        c1 += gv[j][i];
        c2 = fmaf(gv[j][i], xh, c2);
        xv[j][i] = xh;
      }
    }
    c1 = wave_sum(c1) * inv_d;
    c2 = wave_sum(c2) * inv_d;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      if (c < nchunk) {
        f32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = in_range ? rstd * (gv[j][i] - c1 - xv[j][i] * c2) : qnan;
        *reinterpret_cast<f32x4*>(dx + t * (int64_t)d + c * 4) = o;
      }
    }
    if (lane == 0) *reinterpret_cast<f32x4*>(stats + 4 * t) = f32x4{pivot, mean, rstd, 0.f};
  }
}

__device__ __forceinline__ float sln_ld(const float* p) { return *p; }
__device__ __forceinline__ float sln_ld(const f16* p) { return (float)*p; }
__device__ __forceinline__ float sln_ld(const bf16_bits* p) { return bf16_to_f32(*p); }

// Per-bucket column sums of one slab of rows.  Workgroup (blockIdx.x = column tile of 256, blockIdx.y = row slab): thread = column,
// all threads walk the slab's rows together (the row's bucket and statistics are uniform), acc[k][0 / 1][thread] in LDS.
// partial[slab][0][k][col] = sum dy xhat, partial[slab][1][k][col] = sum dy over the slab's rows of bucket k (zeros for none).
template <typename DYT>
__global__ __launch_bounds__(SLN_THREADS) void switch_ln_bwd_cols_kernel(const float* __restrict__ x, const DYT* __restrict__ dy,
                                                                         const int64_t* __restrict__ buckets,
                                                                         const float* __restrict__ stats, int64_t T, int d, int K,
                                                                         int64_t rows_per_slab, float* __restrict__ partial) {
  extern __shared__ float sln_acc[];            // [K][2][SLN_THREADS]
  const int tid = threadIdx.x;
  const int col = blockIdx.x * SLN_THREADS + tid;
  const bool live = col < d;
  for (int i = tid; i < K * 2 * SLN_THREADS; i += SLN_THREADS) sln_acc[i] = 0.f;   // (a thread touches its own column only)
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab;
  int64_t r1 = r0 + rows_per_slab;
  if (r1 > T) r1 = T;
  constexpr int U = 4;
  for (int64_t t = r0; t < r1; t += U) {
    float xs[U], ds[U], pivot[U], mean[U], rstd[U];
    int64_t bs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t tt = t + u;
      const bool ok = tt < r1;
      bs[u] = ok ? buckets[tt] : (int64_t)-1;
      pivot[u] = ok ? stats[4 * tt] : 0.f;
      mean[u] = ok ? stats[4 * tt + 1] : 0.f;
      rstd[u] = ok ? stats[4 * tt + 2] : 0.f;
      xs[u] = (ok && live) ? x[tt * (int64_t)d + col] : 0.f;
      ds[u] = (ok && live) ? sln_ld(dy + tt * (int64_t)d + col) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (bs[u] >= 0 && bs[u] < (int64_t)K) {      // uniform over the workgroup
        float* a = sln_acc + ((int)bs[u] * 2) * SLN_THREADS + tid;
        a[0] = fmaf(ds[u], ((xs[u] - pivot[u]) - mean[u]) * rstd[u], a[0]);
        a[SLN_THREADS] += ds[u];
      }
    }
  }
  if (live) {
    float* p = partial + (int64_t)blockIdx.y * 2 * K * d;
    for (int k = 0; k < K; ++k) {
      p[(int64_t)k * d + col] = sln_acc[(k * 2) * SLN_THREADS + tid];
      p[(int64_t)(K + k) * d + col] = sln_acc[(k * 2 + 1) * SLN_THREADS + tid];
    }
  }
}

// row slabs of the column pass: 16 rows at least per slab, at most 4 workgroups per CU over all column tiles
inline int sln_slabs(int64_t T, int d) {
  const int tiles = (d + SLN_THREADS - 1) / SLN_THREADS;
  int64_t need = (T + 15) / 16;
  int64_t cap = (int64_t)smoe_num_cus() * 4 / tiles;
  if (cap < 1) cap = 1;
  if (need > cap) need = cap;
  return (int)(need < 1 ? 1 : need);
}

inline size_t sln_stats_floats(int64_t T) { return (size_t)T * 4; }      // (pivot, mean - pivot, rstd, -) per row

inline bool sln_shape_ok(int d, int K) { return d >= 4 && d <= 1024 && d % 4 == 0 && K >= 1 && K <= SLN_MAX_K; }

template <int NJ, int KP>
int sln_fwd_launch(bool big, int grid, hipStream_t s, const float* x, const float* weights, const float* biases,
                   const float* centroids, const int64_t* buckets_in, int bucket_all, float eps, int64_t T, int d, int K, float* y,
                   int64_t* buckets_out) {
  const size_t lds = KP > 0 ? (size_t)K * d * sizeof(float) : 0;
  if constexpr (KP >= 16) {        // (K d > SLN_LDS_FLOATS needs K >= 13)
    if (big) {
      SMOE_ENSURE_SMEM(switch_ln_fwd_kernel<NJ, KP, SLN_BIG_THREADS>);
      hipLaunchKernelGGL((switch_ln_fwd_kernel<NJ, KP, SLN_BIG_THREADS>), dim3(grid), dim3(SLN_BIG_THREADS), lds, s, x, weights, biases,
                         centroids, buckets_in, bucket_all, eps, T, d, K, y, buckets_out);
      return 0;
    }
  }
  hipLaunchKernelGGL((switch_ln_fwd_kernel<NJ, KP, SLN_THREADS>), dim3(grid), dim3(SLN_THREADS), lds, s, x, weights, biases, centroids,
                     buckets_in, bucket_all, eps, T, d, K, y, buckets_out);
  return 0;
}

template <int NJ>
int sln_fwd_kp(int kp, bool big, int grid, hipStream_t s, const float* x, const float* weights, const float* biases,
               const float* centroids, const int64_t* buckets_in, int bucket_all, float eps, int64_t T, int d, int K, float* y,
               int64_t* buckets_out) {
#define SLN_F(KP) return sln_fwd_launch<NJ, KP>(big, grid, s, x, weights, biases, centroids, buckets_in, bucket_all, eps, T, d, K, y, buckets_out)
  switch (kp) {
    case 0: SLN_F(0);
    case 2: SLN_F(2);
    case 4: SLN_F(4);
    case 8: SLN_F(8);
    case 16: SLN_F(16);
    default: SLN_F(32);
  }
#undef SLN_F
}

template <typename DYT>
int sln_bwd_launch(const float* x, const void* dyv, const float* weights, const int64_t* buckets, float eps, int64_t T, int d, int K,
                   float* dx, float* dweights, float* dbiases, float* ws, hipStream_t s) {
  const DYT* dy = (const DYT*)dyv;
  float* stats = ws;
  float* partial = ws + sln_stats_floats(T);
  const int grid = wr4_grid(T, SLN_WAVES, 4);
  const bool ok = wr4_dispatch_nj((d / 4 + 63) / 64, [&](auto nj) {
    hipLaunchKernelGGL((switch_ln_bwd_dx_kernel<DYT, decltype(nj)::value>), dim3(grid), dim3(SLN_THREADS), 0, s, x, dy, weights, buckets,
                       eps, T, d, K, dx, stats);
  });
  if (!ok) { smoe_set_error("smoe_switch_ln_bwd: d=%d out of range (d <= 1024)", d); return 1; }
  SMOE_CHECK_LAUNCH("smoe_switch_ln_bwd/dx");
  if (!dweights) return 0;
  const int slabs = sln_slabs(T, d), tiles = (d + SLN_THREADS - 1) / SLN_THREADS;
  const int64_t rows_per_slab = (T + slabs - 1) / slabs;
  const int L = 2 * K * d;
  hipLaunchKernelGGL((switch_ln_bwd_cols_kernel<DYT>), dim3(tiles, slabs), dim3(SLN_THREADS), (size_t)K * 2 * SLN_THREADS * sizeof(float),
                     s, x, dy, buckets, stats, T, d, K, rows_per_slab, partial);
  SMOE_CHECK_LAUNCH("smoe_switch_ln_bwd/cols");
  wr4_reduce_partials(partial, slabs, L, dweights, K * d, dbiases, s);     // the last stage writes dweights and dbiases apart
  SMOE_CHECK_LAUNCH("smoe_switch_ln_bwd/reduce");
  return 0;
}

}  // namespace

extern "C" int smoe_switch_ln_supported(int d, int K) { return sln_shape_ok(d, K) ? 1 : 0; }

extern "C" int smoe_switch_ln_fwd(const float* x, const float* weights, const float* biases, const float* centroids,
                                  const int64_t* buckets_in, int bucket_all, float eps, int64_t T, int d, int K, float* y,
                                  int64_t* buckets_out, void* stream) {
  SMOE_REQUIRE(T >= 0 && sln_shape_ok(d, K), "smoe_switch_ln_fwd: unsupported shape T=%lld d=%d K=%d (d %% 4 == 0, d <= 1024, 1 <= K <= 32)",
               (long long)T, d, K);
  SMOE_REQUIRE((weights != nullptr) || (biases == nullptr), "smoe_switch_ln_fwd: biases without weights");
  SMOE_REQUIRE(bucket_all >= -1, "smoe_switch_ln_fwd: bucket_all must be -1 (unused) or a bucket");
  SMOE_REQUIRE(!(buckets_in && bucket_all >= 0), "smoe_switch_ln_fwd: buckets_in and bucket_all are exclusive");
  const bool select = !buckets_in && bucket_all < 0 && K > 1;
  SMOE_REQUIRE(!select || centroids, "smoe_switch_ln_fwd: centroids needed to select among K > 1 buckets");
  if (T == 0) return 0;
  SMOE_REQUIRE(x && y && buckets_out, "smoe_switch_ln_fwd: null pointer");
  SMOE_REQUIRE(((uintptr_t)x | (uintptr_t)y | (uintptr_t)weights | (uintptr_t)biases | (uintptr_t)(select ? centroids : nullptr)) % 16 == 0,
               "smoe_switch_ln_fwd: x, y and the tables must be 16-byte aligned");
  SMOE_REQUIRE(((uintptr_t)buckets_in | (uintptr_t)buckets_out) % 8 == 0, "smoe_switch_ln_fwd: bucket arrays must be 8-byte aligned");
  if (!buckets_in && bucket_all < 0 && K == 1) bucket_all = 0;     // one bucket: nothing to select, the centroids are never read
  int kp = 0;
  if (select) { kp = 2; while (kp < K) kp *= 2; }
  const bool big = select && K * d > SLN_LDS_FLOATS;
  // several SLN_THREADS-wide workgroups per CU, or one workgroup of 16 waves per CU
  const int grid = big ? wr4_grid(T, SLN_BIG_THREADS / 64, 1) : wr4_grid(T, SLN_WAVES, 8);
  hipStream_t s = (hipStream_t)stream;
  const float* cent = select ? centroids : nullptr;
  int rc = 0;
  const bool ok = wr4_dispatch_nj((d / 4 + 63) / 64, [&](auto nj) {
    rc = sln_fwd_kp<decltype(nj)::value>(kp, big, grid, s, x, weights, biases, cent, buckets_in, bucket_all, eps, T, d, K, y, buckets_out);
  });
  if (!ok) { smoe_set_error("smoe_switch_ln_fwd: d=%d out of range (d <= 1024)", d); return 1; }
  if (rc != 0) return rc;
  SMOE_CHECK_LAUNCH("smoe_switch_ln_fwd");
  return 0;
}

extern "C" size_t smoe_switch_ln_bwd_workspace_bytes(int64_t T, int d, int K) {
  if (T < 0 || !sln_shape_ok(d, K)) return 0;
  return (sln_stats_floats(T) + ((size_t)sln_slabs(T, d) + WR4_STAGE1) * 2 * (size_t)K * d) * sizeof(float);
}

extern "C" int smoe_switch_ln_bwd(const float* x, const void* dy, int dy_dtype, const float* weights, const int64_t* buckets,
                                  float eps, int64_t T, int d, int K, float* dx, float* dweights, float* dbiases, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  SMOE_REQUIRE(T >= 0 && sln_shape_ok(d, K), "smoe_switch_ln_bwd: unsupported shape T=%lld d=%d K=%d (d %% 4 == 0, d <= 1024, 1 <= K <= 32)",
               (long long)T, d, K);
  SMOE_REQUIRE(smoe_dtype_ok(dy_dtype), "smoe_switch_ln_bwd: bad dy dtype");
  SMOE_REQUIRE((dweights != nullptr) == (dbiases != nullptr), "smoe_switch_ln_bwd: dweights and dbiases come together");
  SMOE_REQUIRE(workspace && workspace_bytes >= smoe_switch_ln_bwd_workspace_bytes(T, d, K), "smoe_switch_ln_bwd: workspace too small");
  SMOE_REQUIRE(T == 0 || (x && dy && dx && buckets), "smoe_switch_ln_bwd: null pointer");
  SMOE_REQUIRE(((uintptr_t)x | (uintptr_t)dx | (uintptr_t)weights | (uintptr_t)workspace) % 16 == 0 &&
                   (uintptr_t)dy % (dy_dtype == SMOE_F32 ? 16 : 8) == 0 && (uintptr_t)buckets % 8 == 0,
               "smoe_switch_ln_bwd: misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  float* ws = reinterpret_cast<float*>(workspace);
  switch (dy_dtype) {
    case SMOE_F32: return sln_bwd_launch<float>(x, dy, weights, buckets, eps, T, d, K, dx, dweights, dbiases, ws, s);
    case SMOE_F16: return sln_bwd_launch<f16>(x, dy, weights, buckets, eps, T, d, K, dx, dweights, dbiases, ws, s);
    default: return sln_bwd_launch<bf16_bits>(x, dy, weights, buckets, eps, T, d, K, dx, dweights, dbiases, ws, s);
  }
}
