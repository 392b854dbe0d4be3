// The recipe around the model in the reference's training step (engine.py:46-47, 54: `samples, targets = mixup_fn(samples, targets)`,
// `loss = criterion(samples, outputs, targets)`; main.py:505-517 timm.data.Mixup, main.py:653-661 timm.loss.SoftTargetCrossEntropy /
// LabelSmoothingCrossEntropy; the default run is --mixup 0.8 --cutmix 1.0 --smoothing 0.1):
//   smoe_mixup_images : Mixup / CutMix of a batch IN PLACE, one read and one write of every image (upstream: a flipped copy and three
//                       in-place passes), bit-equal to timm's lines in all three of its modes
//   smoe_mixup_target : the mixed, smoothed one-hot targets in one launch (upstream: eight)
//   smoe_soft_ce_fwd  : mean over rows of sum(-t * log_softmax(x)) for dense targets, or of the label-smoothing loss for integer
//                       labels; one online max / sum pass per row + a fixed-order sum of the row losses (deterministic)
//   smoe_soft_ce_bwd  : dlogits = g (softmax(x) sum(t) - t) / B in the logits' dtype, g a device scalar (it carries the loss scale)
// and the criterion every run of the reference ends in (main.py:688 DistillationLoss; losses.py:53-72):
//   smoe_distill_fwd  : the distillation term between the student's distillation logits and a teacher's logits -- soft: KL(teacher ||
//                       student) at temperature tau; hard: cross-entropy against the teacher's argmax -- and its blend with the base loss
//   smoe_distill_bwd  : its gradient for the student's distillation logits (the teacher gets none)
// and the criterion of --bce-loss (main.py:663-664 torch.nn.BCEWithLogitsLoss, with engine.py:49-50's `targets.gt(0.0)` folded in):
//   smoe_bce_fwd      : mean over all elements of max(x, 0) - x t + log1p(exp(-|x|)); a row sum per workgroup + a fixed-order mean
//   smoe_bce_bwd      : dlogits = g (sigmoid(x) - t) / (B C) in the logits' dtype, element-wise
// and what the reference's evaluate() computes after every forward (engine.py:99-113):
//   smoe_eval_metrics : per-row cross-entropy + the label's rank in one pass, then the batch's loss / top-k accuracies and an f64
//                       accumulator for the epoch, all on the device (upstream: a dozen launches and three host reads)
// Shared by the criteria: wave_sum / tree4 and MaxSum's tree4 (the block reduction's two halves), MaxSumD::merge, and with_dtype /
// with_vec (from dtype codes and alignment to a kernel instantiation).  DESIGN.md, "The loss family's shared pieces".
#include "smoe_common.h"
#include <type_traits>

namespace {

constexpr int LOSS_THREADS = 256;
constexpr int MIX_UNROLL = 4;     // vectors (or single elements on the scalar path) per thread of the image kernel

// ---- Mixup / CutMix of the images ------------------------------------------------------------------------------------------
// what one sample of a pair does with its own value a and its partner's value c at a position (y, x)
struct MixRule {
  float lam, om;
  int yl, yh, xl, xh;
  bool same, cut;      // same: lam == 1, the sample is left as it is; cut: a non-empty box (CutMix), else Mixup
  __device__ __forceinline__ bool inside(int y, int x) const { return y >= yl && y < yh && x >= xl && x < xh; }
  __device__ __forceinline__ float apply(float a, float c, int y, int x) const {
    if (same) return a;
    if (cut) return inside(y, x) ? c : a;
    return __fadd_rn(__fmul_rn(a, lam), __fmul_rn(c, om));     // three roundings, as torch's x * lam + x_flipped * (1 - lam)
  }
};

__device__ __forceinline__ MixRule mix_rule(const float* lam, const float* om, const int32_t* box, int b) {
  MixRule r;
  r.lam = lam[b]; r.om = om[b];
  r.yl = box[4 * b]; r.yh = box[4 * b + 1]; r.xl = box[4 * b + 2]; r.xh = box[4 * b + 3];
  r.same = r.lam == 1.0f;
  r.cut = r.yh > r.yl && r.xh > r.xl;
  return r;
}

// One workgroup set per PAIR (b, B-1-b): a thread loads position p of both images, computes both outputs from the two originals
// and stores both -- correct in place whatever the two samples of the pair do.  VEC = 4: 16 bytes per lane and image (n % 4 == 0 and
// a 16-byte aligned base); VEC = 1: everything else.  A pair without a Mixup sample touches only the positions inside its boxes.
template <int VEC>
__global__ __launch_bounds__(LOSS_THREADS) void mixup_images_kernel(float* __restrict__ x, int B, uint32_t n, int H, int W,
                                                                     const float* __restrict__ lam, const float* __restrict__ om,
                                                                     const int32_t* __restrict__ box) {
  const int b = blockIdx.y, j = B - 1 - b;
  const MixRule rb = mix_rule(lam, om, box, b), rj = mix_rule(lam, om, box, j);
  if (rb.same && rj.same) return;
  const bool sparse = (rb.same || rb.cut) && (rj.same || rj.cut);    // no full pass: only box positions change
  const bool need_pos = rb.cut || rj.cut;
  float* __restrict__ xb = x + (size_t)b * n;
  float* __restrict__ xj = x + (size_t)j * n;
  const uint32_t hw = (uint32_t)H * (uint32_t)W;
  const uint32_t base = blockIdx.x * (uint32_t)(LOSS_THREADS * VEC * MIX_UNROLL) + threadIdx.x * VEC;
  float a[MIX_UNROLL][VEC], c[MIX_UNROLL][VEC];
  int py[MIX_UNROLL], px[MIX_UNROLL];
  bool live[MIX_UNROLL];
#pragma unroll
  for (int u = 0; u < MIX_UNROLL; ++u) {
    const uint32_t p = base + u * (uint32_t)(LOSS_THREADS * VEC);
    live[u] = p < n;      // (VEC = 4: n % 4 == 0, so a live vector is whole)
    py[u] = px[u] = 0;
    if (live[u] && need_pos) {
      const uint32_t rem = p % hw;
      py[u] = (int)(rem / (uint32_t)W);
      px[u] = (int)(rem - (uint32_t)py[u] * (uint32_t)W);
    }
    if (live[u] && sparse) {
      // the VEC positions from (py, px) on lie in rows py and (when the vector crosses a row end) the following ones
      bool any = false;
      int y = py[u], xx = px[u];
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        any |= (rb.cut && !rb.same && rb.inside(y, xx)) || (rj.cut && !rj.same && rj.inside(y, xx));
        if (++xx == W) { xx = 0; if (++y == H) y = 0; }
      }
      live[u] = any;
    }
    if (live[u]) {
      if constexpr (VEC == 4) {
        const f32x4 va = *reinterpret_cast<const f32x4*>(xb + p), vc = *reinterpret_cast<const f32x4*>(xj + p);
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[u][q] = va[q]; c[u][q] = vc[q]; }
      } else {
        a[u][0] = xb[p]; c[u][0] = xj[p];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < MIX_UNROLL; ++u) {
    if (!live[u]) continue;
    const uint32_t p = base + u * (uint32_t)(LOSS_THREADS * VEC);
    float ob[VEC], oj[VEC];
    int y = py[u], xx = px[u];
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      ob[q] = rb.apply(a[u][q], c[u][q], y, xx);
      oj[q] = rj.apply(c[u][q], a[u][q], y, xx);
      if (++xx == W) { xx = 0; if (++y == H) y = 0; }
    }
    if constexpr (VEC == 4) {
      f32x4 vb, vj;
#pragma unroll
      for (int q = 0; q < 4; ++q) { vb[q] = ob[q]; vj[q] = oj[q]; }
      if (!rb.same) *reinterpret_cast<f32x4*>(xb + p) = vb;
      if (!rj.same) *reinterpret_cast<f32x4*>(xj + p) = vj;
    } else {
      if (!rb.same) xb[p] = ob[0];
      if (!rj.same) xj[p] = oj[0];
    }
  }
}

// out[b, c] = one_hot(labels[b])[c] * lam[b] + one_hot(labels[B-1-b])[c] * om[b], three roundings (timm's mixup_target)
__global__ __launch_bounds__(LOSS_THREADS) void mixup_target_kernel(const int64_t* __restrict__ labels, const float* __restrict__ lam,
                                                                    const float* __restrict__ om, float on, float off, int B, int C,
                                                                    float* __restrict__ out) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int64_t l1 = labels[b], l2 = labels[B - 1 - b];
    const float la = lam[b], lo = om[b];
    const int c = blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (c < C) out[(size_t)b * C + c] = __fadd_rn(__fmul_rn(c == l1 ? on : off, la), __fmul_rn(c == l2 ? on : off, lo));
  }
}

// ---- soft-target / label-smoothing cross-entropy ---------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ float to_f32(T v) {
  if constexpr (std::is_same<T, bf16_bits>::value) return bf16_to_f32(v);
  else return (float)v;
}
template <typename T> __device__ __forceinline__ T from_f32(float v) {
  if constexpr (std::is_same<T, bf16_bits>::value) return f32_to_bf16(v);
  else return (T)v;
}

// running (max, sum of exp(x - max)) of a row.  The maximum is never NaN (comparisons drop it), a NaN logit lives on in the sum;
// a -inf logit adds 0; +inf - +inf = NaN poisons the sum, as it does torch's log_softmax.
struct MaxSum {
  float m, s;
  __device__ __forceinline__ void merge(float m2, float s2) {
    const float mm = fmaxf(m, m2);
    s = s * (m == mm ? 1.0f : expf(m - mm)) + s2 * (m2 == mm ? 1.0f : expf(m2 - mm));
    m = mm;
  }
};

constexpr int CE_K = 8;     // logits per thread and step
constexpr int NW = LOSS_THREADS / 64;     // waves of a workgroup

// THE sum of a value (f32, f64, int) over the workgroup, in two halves around the caller's one __syncthreads(): wave_sum
// (smoe_common.h) over the wave, lane 0 of each wave stores it to red[wave], the barrier, then tree4(red) = (w0 + w1) + (w2 + w3) on
// whoever needs it.  Neither half synchronises: a kernel that reduces several values stores them all and synchronises once.
template <typename V> __device__ __forceinline__ V tree4(const V (&red)[NW]) { return (red[0] + red[1]) + (red[2] + red[3]); }
// ... and MaxSum's second half, over the waves' (m, s) as they lie in LDS: the same pairing, (w0, w1), (w2, w3), then the two
__device__ __forceinline__ MaxSum tree4(const float (&rm)[NW], const float (&rs)[NW]) {
  MaxSum a{rm[0], rs[0]}, b{rm[2], rs[2]};
  a.merge(rm[1], rs[1]);
  b.merge(rm[3], rs[3]);
  a.merge(b.m, b.s);
  return a;
}

// compensated (Kahan) sum: a row's targets are one or two values near 1 among thousands near smoothing / C, and the row loss multiplies
// their sum by the log-sum-exp -- a plain running sum's rounding (up to C / 256 half-ulps of 1 per thread) would show there
struct Kahan {
  float s = 0.f, c = 0.f;
  __device__ __forceinline__ void add(float v) {
    const float y = v - c, t = s + y;
    c = (t - s) - y;
    s = t;
  }
};

// K logits of a thread at once (one exp of the running sum per step instead of one per logit)
__device__ __forceinline__ void ce_step(MaxSum& ms, const float (&v)[CE_K], const bool (&ok)[CE_K]) {
  const float ninf = -__builtin_inff();
  float vm = ninf;
#pragma unroll
  for (int q = 0; q < CE_K; ++q) vm = fmaxf(vm, ok[q] ? v[q] : ninf);
  if (vm > ms.m) { ms.s *= expf(ms.m - vm); ms.m = vm; }      // (ms.m == -inf: s is 0 or NaN, and stays that)
  float add = 0.f;
#pragma unroll
  for (int q = 0; q < CE_K; ++q) add += (!ok[q] || v[q] == ninf) ? 0.f : expf(v[q] - ms.m);
  ms.s += add;
}

// One workgroup per row.  Dense form (target != NULL): row loss = lse * sum(t) - dot(t, x).  Label form: t = smoothing / C everywhere
// + (1 - smoothing) at the label (timm LabelSmoothingCrossEntropy; smoothing 0 = cross-entropy), sum(t) = 1.  A label outside [0, C)
// puts the (1 - smoothing) nowhere.  The backward gets the row's maximum and log(sum of exp(x - max)) apart: exp((x - max) - logsum) has
// the error of the small second term only, exp(x - lse) that of lse's rounding.  logsum is stored as NaN whenever the log-sum-exp is not
// finite: the backward then poisons the whole row, as the reference's log_softmax does.
template <typename T, bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void soft_ce_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ target,
                                                                   const int64_t* __restrict__ labels, float smoothing, int C,
                                                                   float* __restrict__ row_loss, float* __restrict__ row_max,
                                                                   float* __restrict__ row_logsum, float* __restrict__ row_tsum) {
  __shared__ float red[4][NW];
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* __restrict__ x = logits + (size_t)row * C;
  const float* __restrict__ t = target ? target + (size_t)row * C : nullptr;
  MaxSum ms{-__builtin_inff(), 0.f};
  Kahan kdot, kts;              // label form: kdot = sum(x)
  const int span = LOSS_THREADS * CE_K;
  for (int c0 = 0; c0 < C; c0 += span) {
    float v[CE_K], tv[CE_K];
    bool ok[CE_K];
    if constexpr (VEC) {     // C % 8 == 0 and aligned bases: 8 consecutive logits (and targets) per lane
      const int c = c0 + tid * CE_K;
      const bool in = c < C;
#pragma unroll
      for (int q = 0; q < CE_K; ++q) { ok[q] = in; v[q] = 0.f; tv[q] = 0.f; }
      if (in) {
        load8(x + c, v);
        if (t) load8(t + c, tv);
      }
    } else {
#pragma unroll
      for (int q = 0; q < CE_K; ++q) {
        const int c = c0 + q * LOSS_THREADS + tid;
        ok[q] = c < C;
        v[q] = ok[q] ? to_f32<T>(x[c]) : 0.f;
        tv[q] = (ok[q] && t) ? t[c] : 0.f;
      }
    }
    ce_step(ms, v, ok);
#pragma unroll
    for (int q = 0; q < CE_K; ++q) {
      if (!ok[q]) continue;
      if (t) { kdot.add(__fmul_rn(tv[q], v[q])); kts.add(tv[q]); }
      else kdot.add(v[q]);
    }
  }
  float dot = kdot.s, ts = kts.s;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float m2 = __shfl_xor(ms.m, m, 64), s2 = __shfl_xor(ms.s, m, 64);
    ms.merge(m2, s2);
    dot += __shfl_xor(dot, m, 64);
    ts += __shfl_xor(ts, m, 64);
  }
  if ((tid & 63) == 0) { red[0][tid >> 6] = ms.m; red[1][tid >> 6] = ms.s; red[2][tid >> 6] = dot; red[3][tid >> 6] = ts; }
  __syncthreads();
  if (tid == 0) {
    const MaxSum a = tree4(red[0], red[1]);
    dot = tree4(red[2]);
    ts = tree4(red[3]);
    float ls = logf(a.s);
    float lse = a.m + ls;
    if (!(fabsf(lse) <= 3.4028234664e38f)) lse = ls = __builtin_nanf("");
    if (!t) {
      const float off = smoothing / (float)C, conf = 1.0f - smoothing;
      const int64_t l = labels[row];
      float d = (l >= 0 && l < C) ? conf * to_f32<T>(x[l]) : 0.f;
      if (smoothing != 0.f) d = fmaf(off, dot, d);
      dot = d;
      ts = 1.0f;
    }
    row_loss[row] = lse * ts - dot;
    row_max[row] = a.m;
    row_logsum[row] = ls;
    row_tsum[row] = ts;
  }
}

// *loss = (sum of row_loss in a fixed order) / B: one workgroup, strided partial sums into wave_sum / tree4 whatever ran before
__global__ __launch_bounds__(LOSS_THREADS) void row_mean_kernel(const float* __restrict__ row_loss, int B, float* __restrict__ loss) {
  __shared__ float red[NW];
  float acc = 0.f;
  for (int r = threadIdx.x; r < B; r += LOSS_THREADS) acc += row_loss[r];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *loss = tree4(red) / (float)B;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void soft_ce_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ target,
                                                                   const int64_t* __restrict__ labels, float smoothing, int B, int C,
                                                                   const float* __restrict__ row_max, const float* __restrict__ row_logsum,
                                                                   const float* __restrict__ row_tsum, const float* __restrict__ g,
                                                                   T* __restrict__ dlogits) {
  const int row = blockIdx.y;
  const size_t at = (size_t)row * C;
  const float mx = row_max[row], ls = row_logsum[row], ts = row_tsum[row], scale = *g / (float)B;
  const float off = smoothing / (float)C, conf = 1.0f - smoothing;
  const int64_t label = target ? -1 : labels[row];
  if constexpr (VEC) {
    const int c = (blockIdx.x * LOSS_THREADS + threadIdx.x) * CE_K;
    if (c >= C) return;
    float v[CE_K], tv[CE_K], o[CE_K];
    load8(logits + at + c, v);
    if (target) load8(target + at + c, tv);
#pragma unroll
    for (int q = 0; q < CE_K; ++q) {
      const float tq = target ? tv[q] : off + (c + q == label ? conf : 0.f);
      o[q] = (expf((v[q] - mx) - ls) * ts - tq) * scale;
    }
    store8(dlogits + at + c, o);
  } else {
#pragma unroll
    for (int q = 0; q < CE_K; ++q) {
      const int c = blockIdx.x * (LOSS_THREADS * CE_K) + q * LOSS_THREADS + threadIdx.x;
      if (c >= C) continue;
      const float tq = target ? target[at + c] : off + (c == label ? conf : 0.f);
      dlogits[at + c] = from_f32<T>((expf((to_f32<T>(logits[at + c]) - mx) - ls) * ts - tq) * scale);
    }
  }
}

// 8 consecutive elements per lane need 16-byte aligned rows of every operand
bool ce_vec_ok(const void* logits, const void* target, const void* dlogits, int C) {
  return C % CE_K == 0 && (((uintptr_t)logits | (uintptr_t)target | (uintptr_t)dlogits) & 15) == 0;
}

constexpr int GRID_Y_MAX = 65535;

// ---- evaluation metrics (engine.py:99-113: criterion, timm's accuracy() and three .item() reads per batch) -------------------------
constexpr int EVAL_MAX_K = 4;
struct TopK { int k[EVAL_MAX_K]; };

// One workgroup per row: soft_ce_fwd_kernel's label form at smoothing 0 -- its loads per thread and its butterfly (written out in
// both kernels: keep them alike), its ce_step and MaxSum's tree4, so row_loss has its bits -- and, on the registers that pass
// holds anyway, the label's rank: the number of classes that come
// before it in a stable descending order where a NaN is the largest value (torch.topk's order; ties go to the lower index).  The
// label's logit x_t is one uniform load up front.  A label outside [0, C): nothing is loaded for it, rank INT32_MAX, loss NaN.
template <typename T, bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void eval_row_kernel(const T* __restrict__ logits, const int64_t* __restrict__ labels, int C,
                                                                float* __restrict__ row_loss, int32_t* __restrict__ row_rank) {
  __shared__ float red[2][NW];
  __shared__ int redc[NW];
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* __restrict__ x = logits + (size_t)row * C;
  const int64_t l = labels[row];
  const bool valid = l >= 0 && l < C;
  const int lab = valid ? (int)l : 0;
  const float xt = valid ? to_f32<T>(x[lab]) : 0.f;
  const bool tn = xt != xt;
  MaxSum ms{-__builtin_inff(), 0.f};
  int cnt = 0;
  const int span = LOSS_THREADS * CE_K;
  for (int c0 = 0; c0 < C; c0 += span) {
    float v[CE_K];
    bool ok[CE_K];
    if constexpr (VEC) {     // C % 8 == 0 and an aligned base: 8 consecutive logits per lane
      const int c = c0 + tid * CE_K;
      const bool in = c < C;
#pragma unroll
      for (int q = 0; q < CE_K; ++q) { ok[q] = in; v[q] = 0.f; }
      if (in) load8(x + c, v);
    } else {
#pragma unroll
      for (int q = 0; q < CE_K; ++q) {
        const int c = c0 + q * LOSS_THREADS + tid;
        ok[q] = c < C;
        v[q] = ok[q] ? to_f32<T>(x[c]) : 0.f;
      }
    }
    ce_step(ms, v, ok);
#pragma unroll
    for (int q = 0; q < CE_K; ++q) {
      const int c = VEC ? c0 + tid * CE_K + q : c0 + q * LOSS_THREADS + tid;
      const bool vn = v[q] != v[q];
      const bool before = !tn && (vn || v[q] > xt);          // x_c comes first whatever its index
      const bool tie = tn ? vn : v[q] == xt;                 // ... or only from a lower index
      cnt += (ok[q] && (before || (tie && c < lab))) ? 1 : 0;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float m2 = __shfl_xor(ms.m, m, 64), s2 = __shfl_xor(ms.s, m, 64);
    ms.merge(m2, s2);
    cnt += __shfl_xor(cnt, m, 64);
  }
  if ((tid & 63) == 0) { red[0][tid >> 6] = ms.m; red[1][tid >> 6] = ms.s; redc[tid >> 6] = cnt; }
  __syncthreads();
  if (tid == 0) {
    const MaxSum a = tree4(red[0], red[1]);
    float lse = a.m + logf(a.s);
    if (!(fabsf(lse) <= 3.4028234664e38f)) lse = __builtin_nanf("");
    row_loss[row] = valid ? lse - xt : __builtin_nanf("");
    row_rank[row] = valid ? tree4(redc) : 0x7fffffff;
  }
}

// One workgroup: batch[0] = the mean of row_loss as row_mean_kernel forms it (the same strided partial sums, butterfly and tree4:
// its bits); batch[1 + i] = (count_i * 100) * f32(1 / B) with
// count_i = #{rows : rank < k_i} -- the f32 operations torch runs ON THE DEVICE for timm's `correct.float().sum() * 100.0 / B` (a
// division by a host scalar is a multiplication by its reciprocal there; measured: a true division differs in 65 of 193 counts at
// B = 192); acc (may be NULL) f64 [2 + nk] +=
// (sum of the row losses in double, B, count_i): a plain read-add-write by one thread, ordered by the stream.  Every sum runs over
// the same strided partial sums and the same tree whatever ran before: the same bits run to run.
__global__ __launch_bounds__(LOSS_THREADS) void eval_batch_kernel(const float* __restrict__ row_loss, const int32_t* __restrict__ row_rank,
                                                                  int B, TopK ks, int nk, float* __restrict__ batch,
                                                                  double* __restrict__ acc) {
  __shared__ float redf[NW];
  __shared__ double redd[NW];
  __shared__ int redc[EVAL_MAX_K][NW];
  float sum = 0.f;
  double dsum = 0.0;
  int cnt[EVAL_MAX_K] = {0, 0, 0, 0};
  for (unsigned r = threadIdx.x; r < (unsigned)B; r += LOSS_THREADS) {
    const float v = row_loss[r];
    const int rk = row_rank[r];
    sum += v;
    dsum += (double)v;
#pragma unroll
    for (int i = 0; i < EVAL_MAX_K; ++i) cnt[i] += (i < nk && rk < ks.k[i]) ? 1 : 0;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sum += __shfl_xor(sum, m, 64);
    dsum += __shfl_xor(dsum, m, 64);
#pragma unroll
    for (int i = 0; i < EVAL_MAX_K; ++i) cnt[i] += __shfl_xor(cnt[i], m, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    redf[w] = sum;
    redd[w] = dsum;
#pragma unroll
    for (int i = 0; i < EVAL_MAX_K; ++i) redc[i][w] = cnt[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    batch[0] = tree4(redf) / (float)B;
    const float inv_b = (float)(1.0 / (double)B);      // torch divides a device tensor by a host scalar as x * f32(1 / B)
    if (acc) {
      acc[0] += tree4(redd);
      acc[1] += (double)B;
    }
    for (int i = 0; i < nk; ++i) {
      const int n = tree4(redc[i]);
      batch[1 + i] = __fmul_rn(__fmul_rn((float)n, 100.f), inv_b);
      if (acc) acc[2 + i] += (double)n;
    }
  }
}

// ---- distillation (losses.py:53-72) -----------------------------------------------------------------------------------------
// The row kernels compute in DOUBLE (MaxSumD / distill_step are MaxSum / ce_step with a double sum): the soft term is a difference of
// nearly equal sums when the student is close to the teacher, and an f32 emulation of its online form on the CPU came out at up to
// 1.8 x the error bar the tests take from torch's own f32 composition (at B = 2 rows, where that bar rests on two samples).  In double
// the arithmetic error is far below one f32 ulp, so what is stored is, to that accuracy, the f64 result rounded to the output type.
// Cost on the GPU: profiles/r10_distillation.md.
constexpr int DISTILL_SOFT = 0, DISTILL_HARD = 1;

// torch.argmax's order: a takes b's place when it is NaN and b is not, when it is greater, or when it ties (two NaNs tie) at a lower index
__device__ __forceinline__ bool argmax_takes(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

// running (max of the raw logits, sum of exp((x - max) / tau)) of a row, the sum in double; MaxSum's rules for non-finite logits: the
// maximum is never NaN, a NaN logit lives on in the sum, a -inf logit adds 0, +inf - +inf = NaN poisons the sum
struct MaxSumD {
  float m;
  double s;
  __device__ __forceinline__ double factor(float mm, double itau) const { return m == mm ? 1.0 : exp(((double)m - (double)mm) * itau); }
  // takes in another partial (m2, s2) ...
  __device__ __forceinline__ void merge(float m2, double s2, double itau) {
    const float mm = fmaxf(m, m2);
    s = s * factor(mm, itau) + s2 * MaxSumD{m2, 0.0}.factor(mm, itau);
    m = mm;
  }
  // ... and with it a second pair of sums (acc, a2) that rides on the same maximum
  __device__ __forceinline__ void merge(float m2, double s2, double& acc, double a2, double itau) {
    const float mm = fmaxf(m, m2);
    const double f1 = factor(mm, itau), f2 = MaxSumD{m2, 0.0}.factor(mm, itau);
    s = s * f1 + s2 * f2;
    acc = acc * f1 + a2 * f2;
    m = mm;
  }
};

// K logits of a thread: ce_step in double.  acc (teacher rows only, with the student's logits in sv): sum of exp((t - max) / tau)
// (t - s) / tau, rescaled with the sum whenever the maximum moves.  Nothing is masked there: a -inf teacher logit gives 0 * -inf = NaN,
// as the reference's exp(log p_t) * (log p_t - log p_s) does.
template <bool KL>
__device__ __forceinline__ void distill_step(MaxSumD& ms, double& acc, const float (&v)[CE_K], const float (&sv)[CE_K],
                                             const bool (&ok)[CE_K], double itau) {
  const float ninf = -__builtin_inff();
  float vm = ninf;
#pragma unroll
  for (int q = 0; q < CE_K; ++q) vm = fmaxf(vm, ok[q] ? v[q] : ninf);
  if (vm > ms.m) {
    const double f = exp(((double)ms.m - (double)vm) * itau);      // (ms.m == -inf: the sums are 0 or NaN, and stay that)
    ms.s *= f;
    if (KL) acc *= f;
    ms.m = vm;
  }
#pragma unroll
  for (int q = 0; q < CE_K; ++q) {
    if (!ok[q]) continue;
    const double e = exp(((double)v[q] - (double)ms.m) * itau);
    ms.s += v[q] == ninf ? 0.0 : e;
    if (KL) acc += e * (((double)v[q] - (double)sv[q]) * itau);
  }
}

// One workgroup per row, both logit rows read once.  soft: s = student / tau, t = teacher / tau, row value = sum p_t (log p_t - log p_s)
// = acc / S_t - (m_t - m_s) / tau - (log S_t - log S_s) with (m, S) the online max / sum of each row.  hard: row value =
// logsumexp(student) - student[argmax teacher], the argmax found in the same pass.  stats f64 [4, B]: the student's maximum (raw) and
// log-sum, the teacher's (soft); a log-sum is stored as NaN when its log-sum-exp is not finite (the backward then poisons the row, as
// the reference's log_softmax does).  label [B]: the argmax (hard), -1 (soft).
template <typename TS, typename TT, bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void distill_fwd_kernel(const TS* __restrict__ student, const TT* __restrict__ teacher, int mode,
                                                                   float tau, int B, int C, double* __restrict__ row_val,
                                                                   double* __restrict__ stats, int32_t* __restrict__ label) {
  __shared__ double redd[3][NW];
  __shared__ float redf[3][NW];
  __shared__ int redi[NW];
  const int row = blockIdx.x, tid = threadIdx.x;
  const TS* __restrict__ x = student + (size_t)row * C;
  const TT* __restrict__ y = teacher + (size_t)row * C;
  const bool hard = mode == DISTILL_HARD;
  const double itau = hard ? 1.0 : 1.0 / (double)tau;
  const float ninf = -__builtin_inff();
  MaxSumD ms{ninf, 0.0}, mt{ninf, 0.0};
  double acc = 0.0;
  float bv = ninf;
  int bi = 0x7fffffff;
  const int span = LOSS_THREADS * CE_K;
  for (int c0 = 0; c0 < C; c0 += span) {
    float sv[CE_K], tv[CE_K];
    bool ok[CE_K];
    // both paths give a thread the same 8 consecutive logits, so the element path (any C, any alignment) computes the vector path's bits
    const int c = c0 + tid * CE_K;
#pragma unroll
    for (int q = 0; q < CE_K; ++q) { ok[q] = c + q < C; sv[q] = 0.f; tv[q] = 0.f; }
    if constexpr (VEC) {     // C % 8 == 0 and 16-byte aligned bases
      if (c < C) { load8(x + c, sv); load8(y + c, tv); }
    } else {
#pragma unroll
      for (int q = 0; q < CE_K; ++q)
        if (ok[q]) { sv[q] = to_f32<TS>(x[c + q]); tv[q] = to_f32<TT>(y[c + q]); }
    }
    distill_step<false>(ms, acc, sv, sv, ok, itau);
    if (hard) {
#pragma unroll
      for (int q = 0; q < CE_K; ++q)
        if (ok[q] && argmax_takes(tv[q], c + q, bv, bi)) { bv = tv[q]; bi = c + q; }
    } else {
      distill_step<true>(mt, acc, tv, sv, ok, itau);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    ms.merge(__shfl_xor(ms.m, m, 64), __shfl_xor(ms.s, m, 64), itau);
    if (hard) {
      const float v2 = __shfl_xor(bv, m, 64);
      const int i2 = __shfl_xor(bi, m, 64);
      if (argmax_takes(v2, i2, bv, bi)) { bv = v2; bi = i2; }
    } else {
      mt.merge(__shfl_xor(mt.m, m, 64), __shfl_xor(mt.s, m, 64), acc, __shfl_xor(acc, m, 64), itau);
    }
  }
  const int w = tid >> 6;
  if ((tid & 63) == 0) {
    redf[0][w] = ms.m; redd[0][w] = ms.s; redf[1][w] = mt.m; redd[1][w] = mt.s; redd[2][w] = acc; redf[2][w] = bv; redi[w] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    MaxSumD a{redf[0][0], redd[0][0]}, t{redf[1][0], redd[1][0]};
    acc = redd[2][0]; bv = redf[2][0]; bi = redi[0];
    for (int k = 1; k < NW; ++k) {
      // (a.merge(redf[0][k], redd[0][k], itau), written out: the form that keeps this loop's LDS reads as they are)
      const float mm = fmaxf(a.m, redf[0][k]);
      a.s = a.s * a.factor(mm, itau) + redd[0][k] * MaxSumD{redf[0][k], 0.0}.factor(mm, itau);
      a.m = mm;
      if (hard) {
        if (argmax_takes(redf[2][k], redi[k], bv, bi)) { bv = redf[2][k]; bi = redi[k]; }
      } else {
        t.merge(redf[1][k], redd[1][k], acc, redd[2][k], itau);
      }
    }
    const double nan = __builtin_nan("");
    double ls = log(a.s), lt = 0.0, tm = 0.0, val;
    if (!(fabs((double)a.m * itau + ls) <= 1.7e308)) ls = nan;
    if (hard) {
      val = ((double)a.m + ls) - (double)to_f32<TS>(x[bi]);       // (C >= 1: bi is an index of the row)
    } else {
      lt = log(t.s);
      tm = (double)t.m;
      val = acc / t.s - ((double)t.m - (double)a.m) * itau - (lt - ls);
      if (!(fabs(tm * itau + lt) <= 1.7e308)) lt = nan;
    }
    row_val[row] = val;
    stats[row] = (double)a.m;
    stats[(size_t)B + row] = ls;
    stats[2 * (size_t)B + row] = tm;
    stats[3 * (size_t)B + row] = lt;
    label[row] = hard ? bi : -1;
  }
}

// *distill = (sum of the row values in a fixed order) * tau^2 / (B C) (soft) or / B (hard); *loss = base (1 - alpha) + distill alpha;
// in double, each rounded to f32 at the store
__global__ __launch_bounds__(LOSS_THREADS) void distill_blend_kernel(const double* __restrict__ row_val, int B, int C, int mode, float tau,
                                                                     float alpha, const float* __restrict__ base,
                                                                     float* __restrict__ distill, float* __restrict__ loss) {
  __shared__ double red[NW];
  double acc = 0.0;
  for (int r = threadIdx.x; r < B; r += LOSS_THREADS) acc += row_val[r];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sum = tree4(red);
    const double d = mode == DISTILL_HARD ? sum / (double)B : sum * ((double)tau * (double)tau) / ((double)B * (double)C);
    *distill = (float)d;
    *loss = (float)((double)*base * (1.0 - (double)alpha) + d * (double)alpha);
  }
}

// soft: dlogits = g alpha tau / (B C) (p_s - p_t);  hard: g alpha / B (p_s - onehot(label)).  p = exp((x - max) / tau - logsum), in double
template <typename TS, typename TT, bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void distill_bwd_kernel(const TS* __restrict__ student, const TT* __restrict__ teacher, int mode,
                                                                   float tau, float alpha, int B, int C, const double* __restrict__ stats,
                                                                   const int32_t* __restrict__ label, const float* __restrict__ g,
                                                                   TS* __restrict__ dlogits) {
  const int row = blockIdx.y;
  const size_t at = (size_t)row * C;
  const bool hard = mode == DISTILL_HARD;
  const double itau = hard ? 1.0 : 1.0 / (double)tau;
  const double ms = stats[row], ls = stats[(size_t)B + row], mt = stats[2 * (size_t)B + row], lt = stats[3 * (size_t)B + row];
  const double scale = hard ? (double)*g * (double)alpha / (double)B
                            : (double)*g * (double)alpha * (double)tau / ((double)B * (double)C);
  const int lab = hard ? label[row] : -1;
  if constexpr (VEC) {
    const int c = (blockIdx.x * LOSS_THREADS + threadIdx.x) * CE_K;
    if (c >= C) return;
    float sv[CE_K], tv[CE_K], o[CE_K];
    load8(student + at + c, sv);
    if (!hard) load8(teacher + at + c, tv);
#pragma unroll
    for (int q = 0; q < CE_K; ++q) {
      const double ps = exp(((double)sv[q] - ms) * itau - ls);
      const double sub = hard ? (c + q == lab ? 1.0 : 0.0) : exp(((double)tv[q] - mt) * itau - lt);
      o[q] = (float)((ps - sub) * scale);
    }
    store8(dlogits + at + c, o);
  } else {
#pragma unroll
    for (int q = 0; q < CE_K; ++q) {
      const int c = blockIdx.x * (LOSS_THREADS * CE_K) + q * LOSS_THREADS + threadIdx.x;
      if (c >= C) continue;
      const double ps = exp(((double)to_f32<TS>(student[at + c]) - ms) * itau - ls);
      const double sub = hard ? (c == lab ? 1.0 : 0.0) : exp(((double)to_f32<TT>(teacher[at + c]) - mt) * itau - lt);
      dlogits[at + c] = from_f32<TS>((float)((ps - sub) * scale));
    }
  }
}

// ---- binary cross-entropy with logits (main.py:663-664 torch.nn.BCEWithLogitsLoss; engine.py:49-50 the target rewrite) ---------------
// the target an element is scored against: engine.py:50's `targets.gt(0.0)` when binarize (-0.0, a negative value and NaN give 0)
__device__ __forceinline__ float bce_target(float t, bool binarize) { return binarize ? (t > 0.f ? 1.f : 0.f) : t; }

// torch's stable form max(x, 0) - x t + log1p(exp(-|x|)).  fmaxf drops a NaN logit, x * t keeps it (NaN * 0 = NaN); an infinite logit
// gives inf or NaN (-inf * 0, inf - inf) under every target: a non-finite logit never gives a finite element.
__device__ __forceinline__ float bce_elem(float x, float t) { return (fmaxf(x, 0.f) - x * t) + log1pf(expf(-fabsf(x))); }

// One workgroup per row: soft_ce_fwd_kernel's columns per thread (8 consecutive elements per lane when VEC, every 256th otherwise),
// the row's sum over the workgroup on wave_sum / tree4.  The elements are f32; their sum runs in double, so that row_loss is the sum of the
// f32 elements rounded once, whatever C is (a row of 1000 elements near 200 would otherwise lose ~log2(C) bits to the running sum).
template <typename T, bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void bce_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ target, int binarize,
                                                               int C, float* __restrict__ row_loss) {
  __shared__ double red[NW];
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* __restrict__ x = logits + (size_t)row * C;
  const float* __restrict__ t = target + (size_t)row * C;
  const bool bin = binarize != 0;
  double acc = 0.0;
  const int span = LOSS_THREADS * CE_K;
  for (int c0 = 0; c0 < C; c0 += span) {
    if constexpr (VEC) {     // C % 8 == 0 and aligned bases: 8 consecutive logits and targets per lane
      const int c = c0 + tid * CE_K;
      if (c < C) {
        float v[CE_K], tv[CE_K];
        load8(x + c, v);
        load8(t + c, tv);
#pragma unroll
        for (int q = 0; q < CE_K; ++q) acc += (double)bce_elem(v[q], bce_target(tv[q], bin));
      }
    } else {
#pragma unroll
      for (int q = 0; q < CE_K; ++q) {
        const int c = c0 + q * LOSS_THREADS + tid;
        if (c < C) acc += (double)bce_elem(to_f32<T>(x[c]), bce_target(t[c], bin));
      }
    }
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) row_loss[row] = (float)tree4(red);
}

// *loss = (sum of row_loss in a fixed order, in double) / (B C), rounded once: reduction='mean' over every element
__global__ __launch_bounds__(LOSS_THREADS) void bce_mean_kernel(const float* __restrict__ row_loss, int B, int C, float* __restrict__ loss) {
  __shared__ double red[NW];
  double acc = 0.0;
  for (int r = threadIdx.x; r < B; r += LOSS_THREADS) acc += (double)row_loss[r];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *loss = (float)(tree4(red) * (1.0 / ((double)B * (double)C)));
}

// sigmoid(x) - t from e = exp(-|x|) in (0, 1]: x >= 0: (1 - t) - e / (1 + e); x < 0: e / (1 + e) - t.  Nothing overflows, and under
// t = 1 a large x gives -e / (1 + e) itself, not 1 - 1.  A NaN or infinite logit, whose loss element is not finite, gives NaN.
__device__ __forceinline__ float bce_grad(float x, float t, float scale) {
  const float e = expf(-fabsf(x));
  const float r = e / (1.0f + e);
  const float d = x >= 0.f ? (1.0f - t) - r : r - t;
  return fabsf(x) <= 3.4028234664e38f ? d * scale : __builtin_nanf("");
}

// purely element-wise: dlogits[b, c] reads logits[b, c], target[b, c] and *g only
template <typename T, bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void bce_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ target, int binarize,
                                                               int B, int C, const float* __restrict__ g, T* __restrict__ dlogits) {
  const size_t at = (size_t)blockIdx.y * C;
  const bool bin = binarize != 0;
  const float scale = (float)((double)*g / ((double)B * (double)C));
  if constexpr (VEC) {
    const int c = (blockIdx.x * LOSS_THREADS + threadIdx.x) * CE_K;
    if (c >= C) return;
    float v[CE_K], tv[CE_K], o[CE_K];
    load8(logits + at + c, v);
    load8(target + at + c, tv);
#pragma unroll
    for (int q = 0; q < CE_K; ++q) o[q] = bce_grad(v[q], bce_target(tv[q], bin), scale);
    store8(dlogits + at + c, o);
  } else {
#pragma unroll
    for (int q = 0; q < CE_K; ++q) {
      const int c = blockIdx.x * (LOSS_THREADS * CE_K) + q * LOSS_THREADS + threadIdx.x;
      if (c >= C) continue;
      dlogits[at + c] = from_f32<T>(bce_grad(to_f32<T>(logits[at + c]), bce_target(target[at + c], bin), scale));
    }
  }
}

// ---- launch dispatch: the element type(s) and VEC of an instantiation from the run-time dtype code(s) and alignment -----------------
// f(tag) with tag a TagF32 / TagF16 / TagBF16 (tag.T is the element type); the entry points have checked the code
template <typename F> void with_dtype(int code, F f) {
  switch (code) {
    case SMOE_F32: f(TagF32{}); break;
    case SMOE_F16: f(TagF16{}); break;
    default: f(TagBF16{}); break;
  }
}
// f(v) with v a std::true_type / std::false_type (v.value is VEC)
template <typename F> void with_vec(bool vec, F f) {
  if (vec) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace

extern "C" int smoe_mixup_images(float* x, int64_t B, int C, int H, int W, const float* lam, const float* one_minus,
                                 const int32_t* box, void* stream) {
  SMOE_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0, "smoe_mixup_images: bad arguments");
  SMOE_REQUIRE(B % 2 == 0, "smoe_mixup_images: the batch size must be even (sample b is mixed with sample B-1-b)");
  const int64_t n = (int64_t)C * H * W;
  SMOE_REQUIRE(n < (1ll << 31) && B / 2 <= GRID_Y_MAX, "smoe_mixup_images: C*H*W < 2^31 and B <= 131070 expected");
  if (B == 0) return 0;
  SMOE_REQUIRE(x && lam && one_minus && box, "smoe_mixup_images: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n % 4 == 0 && ((uintptr_t)x & 15) == 0) {
    const unsigned gx = (unsigned)((n + LOSS_THREADS * 4 * MIX_UNROLL - 1) / (LOSS_THREADS * 4 * MIX_UNROLL));
    hipLaunchKernelGGL(mixup_images_kernel<4>, dim3(gx, (unsigned)(B / 2)), dim3(LOSS_THREADS), 0, s, x, (int)B, (uint32_t)n, H, W, lam, one_minus, box);
  } else {
    const unsigned gx = (unsigned)((n + LOSS_THREADS * MIX_UNROLL - 1) / (LOSS_THREADS * MIX_UNROLL));
    hipLaunchKernelGGL(mixup_images_kernel<1>, dim3(gx, (unsigned)(B / 2)), dim3(LOSS_THREADS), 0, s, x, (int)B, (uint32_t)n, H, W, lam, one_minus, box);
  }
  SMOE_CHECK_LAUNCH("smoe_mixup_images");
  return 0;
}

extern "C" int smoe_mixup_target(const int64_t* labels, const float* lam, const float* one_minus, float on, float off, int64_t B,
                                 int num_classes, float* out, void* stream) {
  SMOE_REQUIRE(B >= 0 && B < (1ll << 31), "smoe_mixup_target: bad arguments");
  SMOE_REQUIRE(num_classes > 0, "smoe_mixup_target: num_classes must be positive");
  if (B == 0) return 0;
  SMOE_REQUIRE(labels && lam && one_minus && out, "smoe_mixup_target: null pointer");
  const dim3 grid((unsigned)((num_classes + LOSS_THREADS - 1) / LOSS_THREADS), (unsigned)(B < GRID_Y_MAX ? B : GRID_Y_MAX));
  hipLaunchKernelGGL(mixup_target_kernel, grid, dim3(LOSS_THREADS), 0, (hipStream_t)stream, labels, lam, one_minus, on, off, (int)B,
                     num_classes, out);
  SMOE_CHECK_LAUNCH("smoe_mixup_target");
  return 0;
}

extern "C" int smoe_soft_ce_fwd(const void* logits, int dtype, const float* target, const int64_t* labels, float smoothing, int64_t B,
                                int C, float* row_loss, float* row_max, float* row_logsum, float* row_tsum, float* loss, void* stream) {
  SMOE_REQUIRE(B >= 0 && B < (1ll << 31) && C > 0 && C <= (1 << 30) && smoe_dtype_ok(dtype), "smoe_soft_ce_fwd: bad arguments (0 < C <= 2^30)");
  SMOE_REQUIRE((target != nullptr) != (labels != nullptr) || B == 0, "smoe_soft_ce_fwd: exactly one of target and labels expected (null pointer)");
  if (B == 0) return 0;
  SMOE_REQUIRE(logits && row_loss && row_max && row_logsum && row_tsum && loss, "smoe_soft_ce_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = ce_vec_ok(logits, target, nullptr, C);
  with_dtype(dtype, [&](auto tag) { with_vec(vec, [&](auto v) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL((soft_ce_fwd_kernel<T, decltype(v)::value>), dim3((unsigned)B), dim3(LOSS_THREADS), 0, s, (const T*)logits, target, labels,
                       smoothing, C, row_loss, row_max, row_logsum, row_tsum);
  }); });
  SMOE_CHECK_LAUNCH("smoe_soft_ce_fwd");
  hipLaunchKernelGGL(row_mean_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, row_loss, (int)B, loss);
  SMOE_CHECK_LAUNCH("smoe_soft_ce_fwd (mean)");
  return 0;
}

extern "C" int smoe_soft_ce_bwd(const void* logits, int dtype, const float* target, const int64_t* labels, float smoothing, int64_t B,
                                int C, const float* row_max, const float* row_logsum, const float* row_tsum, const float* g, void* dlogits, void* stream) {
  SMOE_REQUIRE(B >= 0 && B <= GRID_Y_MAX && C > 0 && C <= (1 << 30) && smoe_dtype_ok(dtype), "smoe_soft_ce_bwd: bad arguments (B <= 65535, 0 < C <= 2^30)");
  SMOE_REQUIRE((target != nullptr) != (labels != nullptr) || B == 0, "smoe_soft_ce_bwd: exactly one of target and labels expected (null pointer)");
  if (B == 0) return 0;
  SMOE_REQUIRE(logits && row_max && row_logsum && row_tsum && g && dlogits, "smoe_soft_ce_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = ce_vec_ok(logits, target, dlogits, C);
  const dim3 grid((unsigned)((C + LOSS_THREADS * CE_K - 1) / (LOSS_THREADS * CE_K)), (unsigned)B);
  with_dtype(dtype, [&](auto tag) { with_vec(vec, [&](auto v) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL((soft_ce_bwd_kernel<T, decltype(v)::value>), grid, dim3(LOSS_THREADS), 0, s, (const T*)logits, target, labels, smoothing,
                       (int)B, C, row_max, row_logsum, row_tsum, g, (T*)dlogits);
  }); });
  SMOE_CHECK_LAUNCH("smoe_soft_ce_bwd");
  return 0;
}

extern "C" int smoe_eval_metrics(const void* logits, int dtype, const int64_t* labels, int64_t B, int C, const int* ks, int nk,
                                 float* row_loss, int32_t* row_rank, float* batch, double* acc, void* stream) {
  SMOE_REQUIRE(B >= 0 && B < (1ll << 31) && C > 0 && C <= (1 << 30), "smoe_eval_metrics: bad sizes (0 <= B < 2^31, 0 < C <= 2^30)");
  SMOE_REQUIRE(smoe_dtype_ok(dtype), "smoe_eval_metrics: bad dtype code %d", dtype);
  SMOE_REQUIRE(nk >= 1 && nk <= EVAL_MAX_K, "smoe_eval_metrics: 1 <= nk <= 4 expected (got %d)", nk);
  SMOE_REQUIRE(ks != nullptr, "smoe_eval_metrics: null pointer (ks, a host array)");
  TopK tk{{0, 0, 0, 0}};
  for (int i = 0; i < nk; ++i) {
    SMOE_REQUIRE(ks[i] >= 1, "smoe_eval_metrics: every k must be >= 1 (ks[%d] = %d)", i, ks[i]);
    tk.k[i] = ks[i];
  }
  if (B == 0) return 0;
  SMOE_REQUIRE(logits && labels && row_loss && row_rank && batch, "smoe_eval_metrics: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = ce_vec_ok(logits, nullptr, nullptr, C);
  with_dtype(dtype, [&](auto tag) { with_vec(vec, [&](auto v) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL((eval_row_kernel<T, decltype(v)::value>), dim3((unsigned)B), dim3(LOSS_THREADS), 0, s, (const T*)logits, labels, C, row_loss,
                       row_rank);
  }); });
  SMOE_CHECK_LAUNCH("smoe_eval_metrics");
  hipLaunchKernelGGL(eval_batch_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, row_loss, row_rank, (int)B, tk, nk, batch, acc);
  SMOE_CHECK_LAUNCH("smoe_eval_metrics (batch)");
  return 0;
}

extern "C" int smoe_distill_fwd(const void* student, int s_dtype, const void* teacher, int t_dtype, int mode, float tau, float alpha,
                                const float* base_loss, int64_t B, int C, double* row_val, double* row_stats, int32_t* row_label,
                                float* distill_loss, float* loss, void* stream) {
  SMOE_REQUIRE(B >= 0 && B < (1ll << 31) && C > 0 && C <= (1 << 30), "smoe_distill_fwd: bad sizes (B < 2^31, 0 < C <= 2^30)");
  SMOE_REQUIRE(smoe_dtype_ok(s_dtype) && smoe_dtype_ok(t_dtype), "smoe_distill_fwd: bad dtype code (student %d, teacher %d)", s_dtype, t_dtype);
  SMOE_REQUIRE(mode == DISTILL_SOFT || mode == DISTILL_HARD, "smoe_distill_fwd: bad mode %d (0 = soft, 1 = hard)", mode);
  SMOE_REQUIRE(tau > 0.f, "smoe_distill_fwd: tau must be positive (got %g)", (double)tau);
  if (B == 0) return 0;
  SMOE_REQUIRE(student && teacher && base_loss && row_val && row_stats && row_label && distill_loss && loss, "smoe_distill_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = ce_vec_ok(student, teacher, nullptr, C);
  with_dtype(s_dtype, [&](auto stag) { with_dtype(t_dtype, [&](auto ttag) { with_vec(vec, [&](auto v) {
    using TS = typename decltype(stag)::T;
    using TT = typename decltype(ttag)::T;
    hipLaunchKernelGGL((distill_fwd_kernel<TS, TT, decltype(v)::value>), dim3((unsigned)B), dim3(LOSS_THREADS), 0, s, (const TS*)student,
                       (const TT*)teacher, mode, tau, (int)B, C, row_val, row_stats, row_label);
  }); }); });
  SMOE_CHECK_LAUNCH("smoe_distill_fwd");
  hipLaunchKernelGGL(distill_blend_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, row_val, (int)B, C, mode, tau, alpha, base_loss, distill_loss, loss);
  SMOE_CHECK_LAUNCH("smoe_distill_fwd (blend)");
  return 0;
}

extern "C" int smoe_distill_bwd(const void* student, int s_dtype, const void* teacher, int t_dtype, int mode, float tau, float alpha,
                                int64_t B, int C, const double* row_stats, const int32_t* row_label, const float* g, void* dlogits,
                                void* stream) {
  SMOE_REQUIRE(B >= 0 && B <= GRID_Y_MAX && C > 0 && C <= (1 << 30), "smoe_distill_bwd: bad sizes (B <= 65535, 0 < C <= 2^30)");
  SMOE_REQUIRE(smoe_dtype_ok(s_dtype) && smoe_dtype_ok(t_dtype), "smoe_distill_bwd: bad dtype code (student %d, teacher %d)", s_dtype, t_dtype);
  SMOE_REQUIRE(mode == DISTILL_SOFT || mode == DISTILL_HARD, "smoe_distill_bwd: bad mode %d (0 = soft, 1 = hard)", mode);
  SMOE_REQUIRE(tau > 0.f, "smoe_distill_bwd: tau must be positive (got %g)", (double)tau);
  if (B == 0) return 0;
  SMOE_REQUIRE(student && teacher && row_stats && row_label && g && dlogits, "smoe_distill_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = ce_vec_ok(student, teacher, dlogits, C);
  const dim3 grid((unsigned)((C + LOSS_THREADS * CE_K - 1) / (LOSS_THREADS * CE_K)), (unsigned)B);
  with_dtype(s_dtype, [&](auto stag) { with_dtype(t_dtype, [&](auto ttag) { with_vec(vec, [&](auto v) {
    using TS = typename decltype(stag)::T;
    using TT = typename decltype(ttag)::T;
    hipLaunchKernelGGL((distill_bwd_kernel<TS, TT, decltype(v)::value>), grid, dim3(LOSS_THREADS), 0, s, (const TS*)student, (const TT*)teacher,
                       mode, tau, alpha, (int)B, C, row_stats, row_label, g, (TS*)dlogits);
  }); }); });
  SMOE_CHECK_LAUNCH("smoe_distill_bwd");
  return 0;
}

extern "C" int smoe_bce_fwd(const void* logits, int dtype, const float* target, int binarize, int64_t B, int C, float* row_loss, float* loss,
                            void* stream) {
  SMOE_REQUIRE(smoe_dtype_ok(dtype), "smoe_bce_fwd: bad dtype code %d", dtype);
  SMOE_REQUIRE(B >= 0 && B <= GRID_Y_MAX && C > 0 && C <= (1 << 30), "smoe_bce_fwd: bad sizes (B <= 65535, 0 < C <= 2^30)");
  if (B == 0) return 0;
  SMOE_REQUIRE(logits && target && row_loss && loss, "smoe_bce_fwd: null pointer");
  SMOE_REQUIRE((uintptr_t)logits % smoe_dtype_size(dtype) == 0 && (((uintptr_t)target | (uintptr_t)row_loss | (uintptr_t)loss) & 3) == 0,
               "smoe_bce_fwd: misaligned pointer (logits to its element size, the f32 buffers to 4 bytes)");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = ce_vec_ok(logits, target, nullptr, C);
  with_dtype(dtype, [&](auto tag) { with_vec(vec, [&](auto v) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL((bce_fwd_kernel<T, decltype(v)::value>), dim3((unsigned)B), dim3(LOSS_THREADS), 0, s, (const T*)logits, target, binarize, C,
                       row_loss);
  }); });
  SMOE_CHECK_LAUNCH("smoe_bce_fwd");
  hipLaunchKernelGGL(bce_mean_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, row_loss, (int)B, C, loss);
  SMOE_CHECK_LAUNCH("smoe_bce_fwd (mean)");
  return 0;
}

extern "C" int smoe_bce_bwd(const void* logits, int dtype, const float* target, int binarize, int64_t B, int C, const float* g, void* dlogits,
                            void* stream) {
  SMOE_REQUIRE(smoe_dtype_ok(dtype), "smoe_bce_bwd: bad dtype code %d", dtype);
  SMOE_REQUIRE(B >= 0 && B <= GRID_Y_MAX && C > 0 && C <= (1 << 30), "smoe_bce_bwd: bad sizes (B <= 65535, 0 < C <= 2^30)");
  if (B == 0) return 0;
  SMOE_REQUIRE(logits && target && g && dlogits, "smoe_bce_bwd: null pointer");
  SMOE_REQUIRE(((uintptr_t)logits | (uintptr_t)dlogits) % smoe_dtype_size(dtype) == 0 && (((uintptr_t)target | (uintptr_t)g) & 3) == 0,
               "smoe_bce_bwd: misaligned pointer (logits and dlogits to their element size, the f32 buffers to 4 bytes)");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = ce_vec_ok(logits, target, dlogits, C);
  const dim3 grid((unsigned)((C + LOSS_THREADS * CE_K - 1) / (LOSS_THREADS * CE_K)), (unsigned)B);
  with_dtype(dtype, [&](auto tag) { with_vec(vec, [&](auto v) {
    using T = typename decltype(tag)::T;
    hipLaunchKernelGGL((bce_bwd_kernel<T, decltype(v)::value>), grid, dim3(LOSS_THREADS), 0, s, (const T*)logits, target, binarize, (int)B, C, g,
                       (T*)dlogits);
  }); });
  SMOE_CHECK_LAUNCH("smoe_bce_bwd");
  return 0;
}
