// LAMB (timm.optim.Lamb, 0.4.12 / 0.5: the DeiT-III recipes' `--opt lamb` / `fusedlamb`, main.py:90-96, 729-731) on the tables of
// the multi-tensor AdamW step (optim.hip): tab = int64 [5][n_t] (p, g, exp_avg, exp_avg_sq addresses and n), blk = int32 [2][n_blocks]
// (tensor of workgroup b, 16K-element block inside it), shadow = int64 [2][n_t] (16-bit image address / dtype), plus
//   hyp   = f32 [3][n_t]   : lr, weight decay, adapt flag (weight_decay != 0 or always_adapt) per tensor
//   first = int32 [n_t + 1]: first block of every tensor (first[n_t] = n_blocks)
// LAMB cannot be one pass: a norm over ALL gradients and two norms per tensor come before any weight moves.  Four launches:
//   smoe_lamb_clip         : block partials of the gradient-norm pass (smoe_grad_sumsq_multi) -> G, clip = max(G / max_grad_norm, 1)
//   smoe_lamb_stage1_multi : moments in place; per block sum(p^2), sum(u^2) of the update u, which stays in registers
//   smoe_lamb_trust_multi  : per tensor r = ||p|| / ||u|| (1 where either is 0, or the tensor does not adapt)
//   smoe_lamb_stage2_multi : u again from the new moments and the old p (lamb_update: the same function, the same bits as stage 1
//                            summed), p -= lr * (r * u), and the 16-bit image of p where there is one
// u is not stored: a parameter-sized f32 buffer costs stage 1 a 4-byte write and stage 2 a 4-byte read per element, the same 8 bytes
// as stage 2 re-reading exp_avg and exp_avg_sq, and would add a third to the optimizer's memory.  Every sum has a fixed order (f32
// inside a block: thread, wave, workgroup; double across blocks), so a step is reproducible bit for bit and a tensor's update does
// not depend on what else is in the launch.  Every kernel returns at once when *found_inf != 0 (GradScaler.step).
#include "optim_table.h"

namespace {

// THE update of one element before the trust ratio: stage 1 sums its square, stage 2 applies it -- one function, so the same bits
__device__ __forceinline__ float lamb_update(float p, float m, float v, float bc1, float bc2_sqrt, float eps, float wd) {
  const float u = (m / bc1) / (sqrtf(v) / bc2_sqrt + eps);
  return wd != 0.f ? fmaf(wd, p, u) : u;
}

// out[0] = clip, out[1] = G = sqrt(sum of the partials) * *num / *den (NULL = 1); max_grad_norm <= 0: no clipping
__global__ __launch_bounds__(OPT_THREADS) void lamb_clip_kernel(const float* __restrict__ partial, int64_t n,
                                                                 const float* __restrict__ num, const float* __restrict__ den,
                                                                 float max_grad_norm, const float* __restrict__ found_inf,
                                                                 float* __restrict__ out) {
  if (found_inf && *found_inf != 0.f) return;
  __shared__ double red[OPT_THREADS];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += OPT_THREADS) acc += (double)partial[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = OPT_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double G = sqrt(red[0]) * (num ? (double)*num : 1.0) / (den ? (double)*den : 1.0);
    out[0] = (max_grad_norm > 0.f && G > (double)max_grad_norm) ? (float)(G / (double)max_grad_norm) : 1.0f;
    out[1] = (float)G;
  }
}

template <typename GT>
__global__ __launch_bounds__(OPT_THREADS) void lamb_stage1_multi_kernel(const int64_t* __restrict__ tab, const float* __restrict__ hyp,
                                                                         int n_t, const int32_t* __restrict__ blk, int64_t n_blocks,
                                                                         double b1d, double b2d, float beta3, float eps,
                                                                         int bias_correction, const float* __restrict__ step,
                                                                         const float* __restrict__ grad_mult,
                                                                         const float* __restrict__ clip,
                                                                         const float* __restrict__ found_inf,
                                                                         float* __restrict__ norms) {
  if (found_inf && *found_inf != 0.f) return;
  int t;
  if (!opt_tensor(blk, n_t, t)) return;
  __shared__ float red[2][OPT_THREADS / 64];
  float* __restrict__ p = opt_row<float, 0>(tab, n_t, t);
  const GT* __restrict__ g = opt_row<const GT, 1>(tab, n_t, t);
  float* __restrict__ m = opt_row<float, 2>(tab, n_t, t);
  float* __restrict__ v = opt_row<float, 3>(tab, n_t, t);
  const int64_t n = opt_entry<4>(tab, n_t, t), base = opt_base(blk, n_blocks), end = opt_end(base, n);
  const float wd = hyp[(int64_t)n_t + t];
  const bool adapt = hyp[2ll * n_t + t] != 0.f;
  const float b1 = (float)b1d, b2 = (float)b2d, one_minus_b2 = (float)(1.0 - b2d);   // (1.0f - 0.999f is off by 1.3e-5 of itself)
  const float gm = (grad_mult ? *grad_mult : 1.0f) / (clip ? *clip : 1.0f);
  float bc1, bc2_sqrt;
  adam_bias(b1d, b2d, *step, bias_correction, bc1, bc2_sqrt);   // *step: already advanced for this update
  float pp = 0.f, uu = 0.f;
  for (int64_t i = base + threadIdx.x * 4; i < end; i += OPT_THREADS * 4) {
    if (i + 4 <= n) {
      float gv[4];
      load4(g + i, gv);
      f32x4 mv = *reinterpret_cast<const f32x4*>(m + i), vv = *reinterpret_cast<const f32x4*>(v + i);
      f32x4 pv = {0.f, 0.f, 0.f, 0.f};
      if (adapt) pv = *reinterpret_cast<const f32x4*>(p + i);   // (a tensor that does not adapt has no weight decay either)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float gq = gv[q] * gm;
        mv[q] = fmaf(mv[q], b1, beta3 * gq);                  // exp_avg.mul_(beta1).add_(grad, alpha=beta3)
        vv[q] = fmaf(vv[q], b2, one_minus_b2 * gq * gq);       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        if (adapt) {
          const float u = lamb_update(pv[q], mv[q], vv[q], bc1, bc2_sqrt, eps, wd);
          pp = fmaf(pv[q], pv[q], pp);
          uu = fmaf(u, u, uu);
        }
      }
      *reinterpret_cast<f32x4*>(m + i) = mv;
      *reinterpret_cast<f32x4*>(v + i) = vv;
    } else {
      for (int64_t j = i; j < n; ++j) {
        const float gq = grad_at<GT>(g, j) * gm;
        const float mj = fmaf(m[j], b1, beta3 * gq), vj = fmaf(v[j], b2, one_minus_b2 * gq * gq);
        m[j] = mj;
        v[j] = vj;
        if (adapt) {
          const float pj = p[j], u = lamb_update(pj, mj, vj, bc1, bc2_sqrt, eps, wd);
          pp = fmaf(pj, pj, pp);
          uu = fmaf(u, u, uu);
        }
      }
    }
  }
  if (!adapt) return;   // (uniform over the workgroup: its trust ratio is 1 and nobody reads its partials)
  wg_sum2_to(pp, uu, red, norms + blockIdx.x, norms + n_blocks + blockIdx.x);
}

// one wave per tensor: its block partials in block order (lane l takes blocks l, l + 64, ...; then the xor tree), in double
__global__ __launch_bounds__(64) void lamb_trust_multi_kernel(const float* __restrict__ norms, int64_t n_blocks,
                                                              const int32_t* __restrict__ first, const float* __restrict__ hyp,
                                                              int n_t, int trust_clip, const float* __restrict__ found_inf,
                                                              float* __restrict__ trust) {
  if (found_inf && *found_inf != 0.f) return;
  const int t = blockIdx.x;
  if (t >= n_t) return;
  if (hyp[2ll * n_t + t] == 0.f) {
    if (threadIdx.x == 0) trust[t] = 1.0f;
    return;
  }
  const int64_t lo = first[t], hi = first[t + 1];
  if (lo < 0 || hi < lo || hi > n_blocks) return;   // the table is caller data
  double w2 = 0.0, u2 = 0.0;
  for (int64_t b = lo + threadIdx.x; b < hi; b += 64) {
    w2 += (double)norms[b];
    u2 += (double)norms[n_blocks + b];
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    w2 += __shfl_xor(w2, s, 64);
    u2 += __shfl_xor(u2, s, 64);
  }
  if (threadIdx.x == 0) {
    const double w = sqrt(w2), u = sqrt(u2);
    float r = (w > 0.0 && u > 0.0) ? (float)(w / u) : 1.0f;
    if (trust_clip && r > 1.0f) r = 1.0f;
    trust[t] = r;
  }
}

__global__ __launch_bounds__(OPT_THREADS) void lamb_stage2_multi_kernel(const int64_t* __restrict__ tab, const float* __restrict__ hyp,
                                                                         int n_t, const int32_t* __restrict__ blk, int64_t n_blocks,
                                                                         double b1d, double b2d, float eps, int bias_correction,
                                                                         const float* __restrict__ step,
                                                                         const float* __restrict__ trust,
                                                                         const float* __restrict__ found_inf,
                                                                         const int64_t* __restrict__ shadow) {
  if (found_inf && *found_inf != 0.f) return;
  int t;
  if (!opt_tensor(blk, n_t, t)) return;
  float* __restrict__ p = opt_row<float, 0>(tab, n_t, t);
  const float* __restrict__ m = opt_row<const float, 2>(tab, n_t, t);
  const float* __restrict__ v = opt_row<const float, 3>(tab, n_t, t);
  const int64_t n = opt_entry<4>(tab, n_t, t), base = opt_base(blk, n_blocks), end = opt_end(base, n);
  const float lr = hyp[t], wd = hyp[(int64_t)n_t + t], r = trust[t];
  void* sh = opt_image(shadow, t);
  const int sh_dtype = opt_image_dtype(shadow, n_t, t);
  float bc1, bc2_sqrt;
  adam_bias(b1d, b2d, *step, bias_correction, bc1, bc2_sqrt);
  for (int64_t i = base + threadIdx.x * 4; i < end; i += OPT_THREADS * 4) {
    if (i + 4 <= n) {
      f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
      const f32x4 mv = *reinterpret_cast<const f32x4*>(m + i), vv = *reinterpret_cast<const f32x4*>(v + i);
#pragma unroll
      for (int q = 0; q < 4; ++q) pv[q] -= lr * (r * lamb_update(pv[q], mv[q], vv[q], bc1, bc2_sqrt, eps, wd));
      *reinterpret_cast<f32x4*>(p + i) = pv;
      image_store4(sh, sh_dtype, i, pv);
    } else {
      for (int64_t j = i; j < n; ++j) {
        const float pj = p[j] - lr * (r * lamb_update(p[j], m[j], v[j], bc1, bc2_sqrt, eps, wd));
        p[j] = pj;
        image_store1(sh, sh_dtype, j, pj);
      }
    }
  }
}

static inline bool lamb_hyper_ok(double beta1, double beta2, float eps) {
  return beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.f;
}

}  // namespace

extern "C" int smoe_lamb_clip(const float* partial, int64_t n_partials, const float* mult_num, const float* mult_den,
                              float max_grad_norm, const float* found_inf, float* out, void* stream) {
  SMOE_REQUIRE(n_partials >= 0 && n_partials < (1ll << 31), "smoe_lamb_clip: bad arguments");
  SMOE_REQUIRE(out && (partial || n_partials == 0), "smoe_lamb_clip: null pointer");
  hipLaunchKernelGGL(lamb_clip_kernel, dim3(1), dim3(OPT_THREADS), 0, (hipStream_t)stream, partial, n_partials, mult_num, mult_den,
                     max_grad_norm, found_inf, out);
  SMOE_CHECK_LAUNCH("smoe_lamb_clip");
  return 0;
}

extern "C" int smoe_lamb_stage1_multi(const int64_t* tab, const float* hyp, int n_tensors, const int32_t* blk, int64_t n_blocks,
                                      int g_dtype, double beta1, double beta2, float beta3, float eps, int bias_correction,
                                      const float* step, const float* grad_mult, const float* clip, const float* found_inf,
                                      float* norms, void* stream) {
  SMOE_REQUIRE(opt_multi_ok(n_tensors, n_blocks, g_dtype) && lamb_hyper_ok(beta1, beta2, eps), "smoe_lamb_stage1_multi: bad arguments");
  if (n_blocks == 0) return 0;
  SMOE_REQUIRE(tab && hyp && blk && step && norms, "smoe_lamb_stage1_multi: null pointer");
  opt_dispatch_grad(g_dtype, [&](auto tag) {
    hipLaunchKernelGGL(lamb_stage1_multi_kernel<typename decltype(tag)::T>, dim3((unsigned)n_blocks), dim3(OPT_THREADS), 0,
                       (hipStream_t)stream, tab, hyp, n_tensors, blk, n_blocks, beta1, beta2, beta3, eps, bias_correction, step, grad_mult,
                       clip, found_inf, norms);
  });
  SMOE_CHECK_LAUNCH("smoe_lamb_stage1_multi");
  return 0;
}

extern "C" int smoe_lamb_trust_multi(const float* norms, int64_t n_blocks, const int32_t* first, const float* hyp, int n_tensors,
                                     int trust_clip, const float* found_inf, float* trust, void* stream) {
  SMOE_REQUIRE(opt_multi_ok(n_tensors, n_blocks), "smoe_lamb_trust_multi: bad arguments");
  if (n_tensors == 0) return 0;
  SMOE_REQUIRE(norms && first && hyp && trust, "smoe_lamb_trust_multi: null pointer");
  hipLaunchKernelGGL(lamb_trust_multi_kernel, dim3((unsigned)n_tensors), dim3(64), 0, (hipStream_t)stream, norms, n_blocks, first, hyp,
                     n_tensors, trust_clip, found_inf, trust);
  SMOE_CHECK_LAUNCH("smoe_lamb_trust_multi");
  return 0;
}

extern "C" int smoe_lamb_stage2_multi(const int64_t* tab, const float* hyp, int n_tensors, const int32_t* blk, int64_t n_blocks,
                                      double beta1, double beta2, float eps, int bias_correction, const float* step,
                                      const float* trust, const float* found_inf, const int64_t* shadow, void* stream) {
  SMOE_REQUIRE(opt_multi_ok(n_tensors, n_blocks) && lamb_hyper_ok(beta1, beta2, eps), "smoe_lamb_stage2_multi: bad arguments");
  if (n_blocks == 0) return 0;
  SMOE_REQUIRE(tab && hyp && blk && step && trust, "smoe_lamb_stage2_multi: null pointer");
  hipLaunchKernelGGL(lamb_stage2_multi_kernel, dim3((unsigned)n_blocks), dim3(OPT_THREADS), 0, (hipStream_t)stream, tab, hyp,
                     n_tensors, blk, n_blocks, beta1, beta2, eps, bias_correction, step, trust, found_inf, shadow);
  SMOE_CHECK_LAUNCH("smoe_lamb_stage2_multi");
  return 0;
}
