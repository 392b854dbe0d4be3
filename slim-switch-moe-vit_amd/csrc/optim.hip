// Optimizer side of the training step (engine.py:68-74 `loss_scaler(loss, optimizer, clip_grad=...,
// parameters=...)` = timm NativeScaler around torch.optim.AdamW, main.py:729-732, --opt adamw): the expert tensors are
// [E,h,d] / [E,d,h] f32 (2 x 75 MB per layer at ViT-B, E = 8) and every pass over them and their gradients is HBM-bound, so
// the step is TWO passes instead of the stock five (unscale, norm, clip-multiply, the optimizer's read and write):
//   smoe_grad_sumsq   : one read of a gradient -> sum of squares of (g * inv_scale) per 16K-element block (deterministic
//                       two-level sum; the caller adds the block partials) and the non-finite flag of GradScaler.unscale_
//   smoe_adamw_step   : decoupled-weight-decay Adam (torch.optim.AdamW arithmetic) reading the STILL-SCALED gradient times
//                       a device-side multiplier (inv_scale x clip coefficient); skipped entirely when found_inf is set;
//                       the step count lives on the device (no host sync anywhere in the step)
//   smoe_amp_update   : GradScaler.update() (growth / backoff of the loss scale) + the optimizer's step counter
//   smoe_ema_update_multi : the weight EMA after the step (timm ModelEma.update), every tensor in one launch, skippable from the device
// LAMB (timm.optim.Lamb: --opt lamb) reads the same tables -- and the block partials of smoe_grad_sumsq_multi -- from lamb.hip.
#include "optim_table.h"

namespace {

// one 16K-element block of one gradient: sum of squares of (g * mul) -> partial[slot]; non-finite -> *found_inf = 1
template <typename GT>
__device__ __forceinline__ void sumsq_block(const GT* __restrict__ g, int64_t n, int64_t block, float mul, float* __restrict__ partial_slot,
                                            float* __restrict__ found_inf) {
  __shared__ float red[OPT_THREADS / 64];
  const int64_t base = block * OPT_BLOCK;
  float acc = 0.f;
  bool bad = false;
  for (int i = threadIdx.x * 8; i < OPT_BLOCK; i += OPT_THREADS * 8) {
    const int64_t at = base + i;
    if (at + 8 <= n) {
      float v[8];
      load8(g + at, v);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float u = v[q] * mul;
        bad |= !(fabsf(u) <= 3.4028234664e38f);   // inf or nan
        acc = fmaf(u, u, acc);
      }
    } else {
      for (int64_t j = at; j < n && j < at + 8; ++j) {
        const float u = grad_at<GT>(g, j) * mul;
        bad |= !(fabsf(u) <= 3.4028234664e38f);
        acc = fmaf(u, u, acc);
      }
    }
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0 && found_inf) *found_inf = 1.0f;
  wg_sum_to(acc, red, partial_slot);
}

template <typename GT>
__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_kernel(const GT* __restrict__ g, int64_t n,
                                                                 const float* __restrict__ inv_scale,
                                                                 float* __restrict__ partial, float* __restrict__ found_inf) {
  sumsq_block<GT>(g, n, blockIdx.x, inv_scale ? *inv_scale : 1.0f, partial + blockIdx.x, found_inf);
}

// MULTI-TENSOR forms: one launch for every gradient / parameter of the step (a ViT-B/16 MoE has ~180 parameter tensors; one
// launch each left the optimizer step bound by launch overhead).  tab = int64 [5][n_t]: rows p, g, m, v (addresses) and n;
// blk = int32 [2][n_blocks]: tensor of workgroup b, 16K-element block inside it (optim_table.h).  Same blocks, same arithmetic,
// same order of the partial sums as the single-tensor forms.
template <typename GT>
__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_multi_kernel(const int64_t* __restrict__ tab, int n_t,
                                                                       const int32_t* __restrict__ blk, int64_t n_blocks,
                                                                       const float* __restrict__ inv_scale,
                                                                       float* __restrict__ partial, float* __restrict__ found_inf) {
  int t;
  if (!opt_tensor(blk, n_t, t)) return;
  sumsq_block<GT>(opt_row<const GT, 1>(tab, n_t, t), opt_entry<4>(tab, n_t, t), blk[n_blocks + blockIdx.x],
                  inv_scale ? *inv_scale : 1.0f, partial + blockIdx.x, found_inf);
}

// torch's lerp(m, g, w = 1 - beta1): m + w (g - m) for w < 0.5, g - (1 - w) (g - m) otherwise
__device__ __forceinline__ float adamw_lerp(float m, float g, float w, float one_minus_w, bool low) {
  const float d = g - m;
  return low ? fmaf(w, d, m) : fmaf(-one_minus_w, d, g);
}

// elements [begin, end) of one parameter, `stride` apart per pass (begin = this thread's first element, a multiple of 4)
// sh (optional): a 16-bit image of the parameter (the MFMA operand copy the forward reads), refreshed in the same pass -- the step
// then needs no separate f32 -> 16-bit cast of every weight (4 bytes read + 2 written per element) before the next forward
template <typename GT>
__device__ __forceinline__ void adamw_range(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int64_t begin, int64_t end, int64_t stride, int64_t n, float lr,
                                            double b1d, double b2d, float eps, float wd, float t, float gm, void* sh = nullptr,
                                            int sh_dtype = SMOE_F16) {
  // every factor that holds 1 - beta comes from the double betas, rounded once (smoe_common.h)
  const float b1 = (float)b1d, b2 = (float)b2d, one_minus_b1 = (float)(1.0 - b1d), one_minus_b2 = (float)(1.0 - b2d);
  const bool low = one_minus_b1 < 0.5f;   // torch's lerp: from the end the weight is nearer to (beta1 = 0: exp_avg = g exactly)
  float bc1, bc2_sqrt;
  adam_bias(b1d, b2d, t, 1, bc1, bc2_sqrt);
  const float step_size = lr / bc1, decay = 1.0f - lr * wd;
  for (int64_t i = begin; i < end; i += stride) {
    if (i + 4 <= n) {
      float gv[4];
      load4(g + i, gv);
      f32x4 pv = *reinterpret_cast<f32x4*>(p + i), mv = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float gq = gv[q] * gm;
        pv[q] *= decay;
        mv[q] = adamw_lerp(mv[q], gq, one_minus_b1, b1, low);   // exp_avg.lerp_(grad, 1 - beta1)
        vv[q] = fmaf(vv[q], b2, one_minus_b2 * gq * gq);        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        const float denom = sqrtf(vv[q]) / bc2_sqrt + eps;
        pv[q] -= step_size * (mv[q] / denom);
      }
      *reinterpret_cast<f32x4*>(p + i) = pv;
      *reinterpret_cast<f32x4*>(m + i) = mv;
      *reinterpret_cast<f32x4*>(v + i) = vv;
      image_store4(sh, sh_dtype, i, pv);
    } else {
      for (int64_t j = i; j < n; ++j) {
        const float gq = grad_at<GT>(g, j) * gm;
        float pj = p[j] * decay, mj = adamw_lerp(m[j], gq, one_minus_b1, b1, low), vj = fmaf(v[j], b2, one_minus_b2 * gq * gq);
        pj -= step_size * (mj / (sqrtf(vj) / bc2_sqrt + eps));
        p[j] = pj; m[j] = mj; v[j] = vj;
        image_store1(sh, sh_dtype, j, pj);
      }
    }
  }
}

template <typename GT>
__global__ __launch_bounds__(OPT_THREADS) void adamw_kernel(float* __restrict__ p, const GT* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                            double b1, double b2, float eps, float wd,
                                                            const float* __restrict__ step, const float* __restrict__ grad_mult,
                                                            const float* __restrict__ found_inf) {
  if (found_inf && *found_inf != 0.f) return;   // GradScaler.step: a non-finite gradient skips the whole update
  // *step: already advanced for this update
  adamw_range<GT>(p, g, m, v, ((int64_t)blockIdx.x * OPT_THREADS + threadIdx.x) * 4, n, (int64_t)gridDim.x * OPT_THREADS * 4, n,
                  lr, b1, b2, eps, wd, *step, grad_mult ? *grad_mult : 1.0f);
}

// hyp = f32 [2][n_t]: lr, weight decay per tensor (parameter groups differ in both)
template <typename GT>
__global__ __launch_bounds__(OPT_THREADS) void adamw_multi_kernel(const int64_t* __restrict__ tab, const float* __restrict__ hyp,
                                                                  int n_t, const int32_t* __restrict__ blk, int64_t n_blocks,
                                                                  double b1, double b2, float eps, const float* __restrict__ step,
                                                                  const float* __restrict__ grad_mult,
                                                                  const float* __restrict__ found_inf,
                                                                  const int64_t* __restrict__ shadow) {
  if (found_inf && *found_inf != 0.f) return;
  int t;
  if (!opt_tensor(blk, n_t, t)) return;
  const int64_t n = opt_entry<4>(tab, n_t, t), base = opt_base(blk, n_blocks);
  adamw_range<GT>(opt_row<float, 0>(tab, n_t, t), opt_row<const GT, 1>(tab, n_t, t), opt_row<float, 2>(tab, n_t, t),
                  opt_row<float, 3>(tab, n_t, t), base + threadIdx.x * 4, opt_end(base, n), OPT_THREADS * 4, n, hyp[t], b1, b2, eps,
                  hyp[n_t + t], *step, grad_mult ? *grad_mult : 1.0f, opt_image(shadow, t), opt_image_dtype(shadow, n_t, t));
}

// weight EMA (timm.utils.ModelEma.update: `ema_v.copy_(ema_v * decay + (1. - decay) * model_v)`, engine.py:77-78), in place.
// tab = int64 [3][n_t]: rows ema, model (addresses, f32) and n; blk as above.  Bit-equal to torch's line: three separately
// rounded f32 operations with the two host-side factors f32(decay) and f32(1 - decay) (the latter computed in double) -- the
// _rn intrinsics keep -ffp-contract=on from fusing them into an FMA.
__global__ __launch_bounds__(OPT_THREADS) void ema_update_multi_kernel(const int64_t* __restrict__ tab, int n_t,
                                                                       const int32_t* __restrict__ blk, int64_t n_blocks,
                                                                       float decay, float one_minus_decay,
                                                                       const float* __restrict__ skip) {
  if (skip && *skip != 0.f) return;
  int t;
  if (!opt_tensor(blk, n_t, t)) return;
  float* __restrict__ e = opt_row<float, 0>(tab, n_t, t);
  const float* __restrict__ m = opt_row<const float, 1>(tab, n_t, t);
  const int64_t n = opt_entry<2>(tab, n_t, t), base = opt_base(blk, n_blocks);
  if (base + OPT_BLOCK <= n) {
    // a whole block: 16 x 16 bytes of each tensor per thread, loads issued EMA_UNROLL vectors at a time (more bytes in flight)
    constexpr int EMA_UNROLL = 4;
    for (int k = 0; k < OPT_BLOCK / (OPT_THREADS * 4); k += EMA_UNROLL) {
      f32x4 ev[EMA_UNROLL], mv[EMA_UNROLL];
#pragma unroll
      for (int u = 0; u < EMA_UNROLL; ++u) {
        const int64_t i = base + (int64_t)(k + u) * OPT_THREADS * 4 + threadIdx.x * 4;
        ev[u] = *reinterpret_cast<const f32x4*>(e + i);
        mv[u] = *reinterpret_cast<const f32x4*>(m + i);
      }
#pragma unroll
      for (int u = 0; u < EMA_UNROLL; ++u) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ev[u][q] = __fadd_rn(__fmul_rn(ev[u][q], decay), __fmul_rn(mv[u][q], one_minus_decay));
        *reinterpret_cast<f32x4*>(e + base + (int64_t)(k + u) * OPT_THREADS * 4 + threadIdx.x * 4) = ev[u];
      }
    }
    return;
  }
  for (int64_t i = base + threadIdx.x * 4; i < n; i += OPT_THREADS * 4) {   // the tensor's last, partial block
    if (i + 4 <= n) {
      f32x4 ev = *reinterpret_cast<const f32x4*>(e + i);
      const f32x4 mv = *reinterpret_cast<const f32x4*>(m + i);
#pragma unroll
      for (int q = 0; q < 4; ++q) ev[q] = __fadd_rn(__fmul_rn(ev[q], decay), __fmul_rn(mv[q], one_minus_decay));
      *reinterpret_cast<f32x4*>(e + i) = ev;
    } else {
      for (int64_t j = i; j < n; ++j) e[j] = __fadd_rn(__fmul_rn(e[j], decay), __fmul_rn(m[j], one_minus_decay));
    }
  }
}

__global__ void amp_update_kernel(float* scale, float* growth_tracker, const float* found_inf, float growth, float backoff,
                                  float interval) {
  if (found_inf && *found_inf != 0.f) {
    *scale *= backoff;
    *growth_tracker = 0.f;
  } else {
    const float tr = *growth_tracker + 1.f;
    if (tr >= interval) {
      *scale *= growth;
      *growth_tracker = 0.f;
    } else {
      *growth_tracker = tr;
    }
  }
}

__global__ void step_advance_kernel(float* step, const float* found_inf) {
  if (!(found_inf && *found_inf != 0.f)) *step += 1.f;
}

}  // namespace

extern "C" int64_t smoe_grad_sumsq_blocks(int64_t n) { return n > 0 ? (n + OPT_BLOCK - 1) / OPT_BLOCK : 0; }

extern "C" int smoe_grad_sumsq(const void* g, int g_dtype, int64_t n, const float* inv_scale, float* partial, float* found_inf,
                               void* stream) {
  SMOE_REQUIRE(n >= 0 && smoe_dtype_ok(g_dtype), "smoe_grad_sumsq: bad arguments");
  if (n == 0) return 0;
  SMOE_REQUIRE(g && partial, "smoe_grad_sumsq: null pointer");
  const int grid = (int)smoe_grad_sumsq_blocks(n);
  hipStream_t s = (hipStream_t)stream;
  opt_dispatch_grad(g_dtype, [&](auto tag) {
    using GT = typename decltype(tag)::T;
    hipLaunchKernelGGL(grad_sumsq_kernel<GT>, dim3(grid), dim3(OPT_THREADS), 0, s, (const GT*)g, n, inv_scale, partial, found_inf);
  });
  SMOE_CHECK_LAUNCH("smoe_grad_sumsq");
  return 0;
}

extern "C" int smoe_adamw_step(float* p, const void* g, int g_dtype, float* m, float* v, int64_t n, float lr, double beta1,
                               double beta2, float eps, float weight_decay, const float* step, const float* grad_mult,
                               const float* found_inf, void* stream) {
  SMOE_REQUIRE(n >= 0 && smoe_dtype_ok(g_dtype), "smoe_adamw_step: bad arguments");
  if (n == 0) return 0;
  SMOE_REQUIRE(p && g && m && v && step, "smoe_adamw_step: null pointer");
  int64_t blocks = (n / 4 + OPT_THREADS - 1) / OPT_THREADS;
  if (blocks < 1) blocks = 1;
  if (blocks > 16384) blocks = 16384;
  hipStream_t s = (hipStream_t)stream;
  opt_dispatch_grad(g_dtype, [&](auto tag) {
    using GT = typename decltype(tag)::T;
    hipLaunchKernelGGL(adamw_kernel<GT>, dim3((int)blocks), dim3(OPT_THREADS), 0, s, p, (const GT*)g, m, v, n, lr, beta1, beta2, eps,
                       weight_decay, step, grad_mult, found_inf);
  });
  SMOE_CHECK_LAUNCH("smoe_adamw_step");
  return 0;
}

extern "C" int smoe_amp_update(float* scale, float* growth_tracker, const float* found_inf, float growth_factor,
                               float backoff_factor, int growth_interval, void* stream) {
  SMOE_REQUIRE(scale && growth_tracker, "smoe_amp_update: null pointer");
  hipLaunchKernelGGL(amp_update_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, scale, growth_tracker, found_inf,
                     growth_factor, backoff_factor, (float)growth_interval);
  SMOE_CHECK_LAUNCH("smoe_amp_update");
  return 0;
}

extern "C" int smoe_step_advance(float* step, const float* found_inf, void* stream) {
  SMOE_REQUIRE(step, "smoe_step_advance: null pointer");
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, found_inf);
  SMOE_CHECK_LAUNCH("smoe_step_advance");
  return 0;
}

extern "C" int smoe_grad_sumsq_multi(const int64_t* tab, int n_tensors, const int32_t* blk, int64_t n_blocks, int g_dtype,
                                     const float* inv_scale, float* partial, float* found_inf, void* stream) {
  SMOE_REQUIRE(opt_multi_ok(n_tensors, n_blocks, g_dtype), "smoe_grad_sumsq_multi: bad arguments");
  if (n_blocks == 0) return 0;
  SMOE_REQUIRE(tab && blk && partial, "smoe_grad_sumsq_multi: null pointer");
  opt_dispatch_grad(g_dtype, [&](auto tag) {
    hipLaunchKernelGGL(grad_sumsq_multi_kernel<typename decltype(tag)::T>, dim3((unsigned)n_blocks), dim3(OPT_THREADS), 0,
                       (hipStream_t)stream, tab, n_tensors, blk, n_blocks, inv_scale, partial, found_inf);
  });
  SMOE_CHECK_LAUNCH("smoe_grad_sumsq_multi");
  return 0;
}

extern "C" int smoe_adamw_step_multi(const int64_t* tab, const float* hyp, int n_tensors, const int32_t* blk, int64_t n_blocks,
                                     int g_dtype, double beta1, double beta2, float eps, const float* step, const float* grad_mult,
                                     const float* found_inf, const int64_t* shadow, void* stream) {
  SMOE_REQUIRE(opt_multi_ok(n_tensors, n_blocks, g_dtype), "smoe_adamw_step_multi: bad arguments");
  if (n_blocks == 0) return 0;
  SMOE_REQUIRE(tab && hyp && blk && step, "smoe_adamw_step_multi: null pointer");
  opt_dispatch_grad(g_dtype, [&](auto tag) {
    hipLaunchKernelGGL(adamw_multi_kernel<typename decltype(tag)::T>, dim3((unsigned)n_blocks), dim3(OPT_THREADS), 0,
                       (hipStream_t)stream, tab, hyp, n_tensors, blk, n_blocks, beta1, beta2, eps, step, grad_mult, found_inf, shadow);
  });
  SMOE_CHECK_LAUNCH("smoe_adamw_step_multi");
  return 0;
}

extern "C" int smoe_ema_update_multi(const int64_t* tab, int n_tensors, const int32_t* blk, int64_t n_blocks, float decay,
                                     float one_minus_decay, const float* skip, void* stream) {
  SMOE_REQUIRE(opt_multi_ok(n_tensors, n_blocks), "smoe_ema_update_multi: bad arguments");
  if (n_blocks == 0) return 0;
  SMOE_REQUIRE(tab && blk, "smoe_ema_update_multi: null pointer");
  hipLaunchKernelGGL(ema_update_multi_kernel, dim3((unsigned)n_blocks), dim3(OPT_THREADS), 0, (hipStream_t)stream, tab, n_tensors,
                     blk, n_blocks, decay, one_minus_decay, skip);
  SMOE_CHECK_LAUNCH("smoe_ema_update_multi");
  return 0;
}
