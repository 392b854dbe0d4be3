// The SOFT token-skip gate of the residual-MoE block in training (models/resMoE.py:72-74: Gate(is_hard=False) replaces the hard masks
// and their straight-through estimator by the relaxation skip_tk = 1 - p, tk = p), forward, fused with the LayerNorm in front of it:
//     xn = LN(x) gamma + beta (or x),  z = <xn, w> + b,  p = sigmoid(z),  tk = xn p,  mask = (1 - p, p)
// ONE pass over x writes the residual image xn32, the operator's input tk as a 16-bit image (attention half) or an f32 image (the MoE
// half's router and scatter) and the mask.  Nothing is decided here, so there is no f64 redo: the layout is wave_row4.h's --
// one wave per row, 16-byte loads per lane, a grid-stride loop under a grid cap, 64-bit row offsets -- and the LayerNorm / logit
// arithmetic is that header's (wr4_row_stats and the xhat / xn expressions it states) with gate_ln_bwd_kernel's logit sum
// (dense_bwd.hip), so the backward recomputes THIS pass's xn and z bit for bit.  At d = 192 a row is 48 sixteen-byte chunks: 16
// lanes of the wave idle.
// Bound: HBM (4 T d bytes read, 4 T d + 2 T d or 4 T d written).
// Skip counter (Gate._skipped_tokens): every wave adds 1 - p of its rows in double, the four waves of a workgroup meet in LDS in wave
// order, every workgroup writes ONE partial sum; a second, one-wave launch adds the partial sums in double in a fixed order (lane l:
// l, l + 64, ... in index order; the lanes in a fixed tree), rounds with rint and adds to the int32 counter.  No atomics, no host
// access.  A row whose 1 - p is NaN (a NaN / inf row) counts as 0: it never poisons the other rows' count.
#include "wave_row4.h"

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_WAVES = SG_THREADS / 64;

template <typename NT> __device__ __forceinline__ void sg_store4_16(NT* dst, const f32x4& v) {   // smoe_gate_ln_router's xn16 conversion
  if constexpr (std::is_same<NT, f16>::value) {
    f16x4 o; o[0] = (f16)v[0]; o[1] = (f16)v[1]; o[2] = (f16)v[2]; o[3] = (f16)v[3];
    *reinterpret_cast<f16x4*>(dst) = o;
  } else {
    s16x4 o; o[0] = (short)f32_to_bf16(v[0]); o[1] = (short)f32_to_bf16(v[1]);
    o[2] = (short)f32_to_bf16(v[2]); o[3] = (short)f32_to_bf16(v[3]);
    *reinterpret_cast<s16x4*>(dst) = o;
  }
}

template <typename NT, int NJ, bool LN>
__global__ __launch_bounds__(SG_THREADS) void soft_gate_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, float eps,
                                                                      const float* __restrict__ gate_w, const float* __restrict__ gate_b,
                                                                      int64_t T, int d, float* __restrict__ xn32, NT* __restrict__ tk16,
                                                                      float* __restrict__ tk32, float* __restrict__ mask,
                                                                      double* __restrict__ partial) {
  __shared__ double red[SG_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = d >> 2;
  f32x4 gm[NJ], bt[NJ], wv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    const bool in = c < nchunk;
    gm[j] = (LN && gamma && in) ? *reinterpret_cast<const f32x4*>(gamma + c * 4) : f32x4{1.f, 1.f, 1.f, 1.f};
    bt[j] = (LN && beta && in) ? *reinterpret_cast<const f32x4*>(beta + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    wv[j] = in ? *reinterpret_cast<const f32x4*>(gate_w + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float bias = gate_b ? *gate_b : 0.f;
  const float inv_d = 1.0f / (float)d;
  double skipped = 0.0;
  const int64_t row0 = (int64_t)blockIdx.x * SG_WAVES + wave, stride = (int64_t)gridDim.x * SG_WAVES;
  for (int64_t t = row0; t < T; t += stride) {
    const int64_t rowoff = t * (int64_t)d;
    float xv[NJ][4];
    wr4_load(nchunk, lane, wr4_row(x + rowoff, xv));
    if constexpr (LN) {   // xv becomes xn, by the steps gate_ln_bwd_kernel recomputes it with
      float mean, rstd;
      wr4_row_stats<false, NJ>(xv, nchunk, lane, inv_d, eps, mean, rstd);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const bool in = lane + 64 * j < nchunk;
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[j][i] = in ? fmaf((xv[j][i] - mean) * rstd, gm[j][i], bt[j][i]) : 0.f;
      }
    }
    float az = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) az = fmaf(xv[j][i], wv[j][i], az);
    const float z = wave_sum(az) + bias;
    // p and 1 - p each as ONE division by 1 + e, e = exp(-|z|): neither is a difference from a rounded value (1 - p taken from the
    // rounded p loses about |z| log2(e) bits once the gate saturates; the e / (1 + e)^2 comment of skip_gate_bwd_kernel)
    const float e = expf(-fabsf(z));
    const float den = 1.0f + e;
    const float hi = 1.0f / den, lo = e / den;
    const bool pos = !(z < 0.f);
    const float p = pos ? hi : lo, om = pos ? lo : hi;
    skipped += (om == om) ? (double)om : 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      if (c < nchunk) {
        f32x4 xn, tk;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xn[i] = xv[j][i];
          float pr = xv[j][i] * p;
          asm volatile("" : "+v"(pr));   // the f32 product is the value: its 16-bit image is a conversion of its own (wave_row_affine)
          tk[i] = pr;
        }
        if (xn32) *reinterpret_cast<f32x4*>(xn32 + rowoff + c * 4) = xn;
        if (tk32) *reinterpret_cast<f32x4*>(tk32 + rowoff + c * 4) = tk;
        if (tk16) sg_store4_16<NT>(tk16 + rowoff + c * 4, tk);
      }
    }
    if (lane == 0 && mask) *reinterpret_cast<f32x2*>(mask + t * 2) = f32x2{om, p};
  }
  if (partial) {   // kernel-uniform
    if (lane == 0) red[wave] = skipped;
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < SG_WAVES; ++w) s += red[w];
      partial[blockIdx.x] = s;
    }
  }
}

// *counter += rint(sum of the n partial sums), one wave
__global__ __launch_bounds__(64) void soft_gate_count_kernel(const double* __restrict__ partial, int n, int32_t* __restrict__ counter) {
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int i = lane; i < n; i += 64) s += partial[i];
  s = wave_sum(s);
  if (lane == 0) *counter += (int32_t)rint(s);
}

inline int sg_grid(int64_t T) { return wr4_grid(T, SG_WAVES, 4); }     // 16 waves per CU, as the backward pass (dense_bwd.hip lnb_grid)

struct SoftGateArgs {
  const float* x; const float* gamma; const float* beta; float eps; const float* gate_w; const float* gate_b;
  int64_t T; int d; float* xn32; void* tk16; float* tk32; float* mask; double* partial; int grid; hipStream_t s;
};

template <typename NT, bool LN> int sg_launch(const SoftGateArgs& a) {   // (a.d is one of the four supported widths)
  const bool ok = wr4_dispatch_nj((a.d / 4 + 63) / 64, [&](auto nj) {
    hipLaunchKernelGGL((soft_gate_ln_fwd_kernel<NT, decltype(nj)::value, LN>), dim3(a.grid), dim3(SG_THREADS), 0, a.s, a.x, a.gamma,
                       a.beta, a.eps, a.gate_w, a.gate_b, a.T, a.d, a.xn32, (NT*)a.tk16, a.tk32, a.mask, a.partial);
  });
  if (!ok) { smoe_set_error("smoe_soft_gate_ln_fwd: unsupported d=%d", a.d); return 1; }
  SMOE_CHECK_LAUNCH("smoe_soft_gate_ln_fwd");
  return 0;
}

}  // namespace

extern "C" int smoe_soft_gate_ln_fwd_supported(int d) { return (d == 192 || d == 384 || d == 768 || d == 1024) ? 1 : 0; }

extern "C" size_t smoe_soft_gate_ln_fwd_workspace_bytes(int64_t T) {
  if (T <= 0) return 0;
  return (size_t)sg_grid(T) * sizeof(double);
}

extern "C" int smoe_soft_gate_ln_fwd(const void* x, int x_dtype, int with_ln, const float* ln_gamma, const float* ln_beta, float ln_eps,
                                     const float* gate_w, const float* gate_b, float* xn32, void* tk16, int tk16_dtype, float* tk32,
                                     float* mask, int32_t* skip_count, int64_t T, int d, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (T == 0) return 0;
  SMOE_REQUIRE(smoe_soft_gate_ln_fwd_supported(d), "smoe_soft_gate_ln_fwd: unsupported d=%d", d);
  SMOE_REQUIRE(x && gate_w, "smoe_soft_gate_ln_fwd: null pointer");
  SMOE_REQUIRE(x_dtype == SMOE_F32, "smoe_soft_gate_ln_fwd: x must be f32 (the residual stream / the normed activations)");
  SMOE_REQUIRE(T > 0 && T < (1ll << 31), "smoe_soft_gate_ln_fwd: bad T");
  SMOE_REQUIRE(tk16_dtype == SMOE_F16 || tk16_dtype == SMOE_BF16, "smoe_soft_gate_ln_fwd: tk16 must be f16 or bf16");
  SMOE_REQUIRE(!skip_count || (workspace && workspace_bytes >= smoe_soft_gate_ln_fwd_workspace_bytes(T) &&
                               ((uintptr_t)workspace & 7) == 0),
               "smoe_soft_gate_ln_fwd: the skip counter needs an 8-byte aligned workspace of smoe_soft_gate_ln_fwd_workspace_bytes(T)");
  SoftGateArgs a{(const float*)x, ln_gamma, ln_beta, ln_eps, gate_w, gate_b, T, d, xn32, tk16, tk32, mask,
                 skip_count ? (double*)workspace : nullptr, sg_grid(T), (hipStream_t)stream};
  int rc;
  switch (((with_ln & 1) ? 2 : 0) | (tk16_dtype == SMOE_BF16 ? 1 : 0)) {
    case 0: rc = sg_launch<f16, false>(a); break;
    case 1: rc = sg_launch<bf16_bits, false>(a); break;
    case 2: rc = sg_launch<f16, true>(a); break;
    default: rc = sg_launch<bf16_bits, true>(a); break;
  }
  if (rc) return rc;
  if (skip_count) {
    hipLaunchKernelGGL(soft_gate_count_kernel, dim3(1), dim3(64), 0, a.s, a.partial, a.grid, skip_count);
    SMOE_CHECK_LAUNCH("smoe_soft_gate_ln_fwd/count");
  }
  return 0;
}
