// Noisy top-k gate (fmoe.gates.NoisyGate, Shazeer et al.; the rule is restated in INTEGRATION.md): the gate's own arithmetic behind
// the unchanged router, which delivers logits2 [T, 2E] = [clean | raw] from the [2E, d] image [w_gate^T ; w_noise^T].
//   smoe_noisy_gate_fwd   sigma = softplus(raw) + 1e-2 (training; 0 in eval), noisy = clean + eps sigma, the k + 1 largest noisy values
//                         of each row (ties -> lowest id) -> idx [T, k], score = softmax over the k kept; importance and load column
//                         sums, aux = cv2(imp) + cv2(load) and the two [E] coefficient vectors d aux / d imp, d aux / d load
//   smoe_noisy_gate_bwd   dlogits2 [T, 2E] of the score and of aux, one pass
// One thread per row (E <= 32: a row of logits2 is at most 256 bytes, walked from L1 -- smoe_gshard_gate_bwd's shape); the k + 1
// best (value, id) pairs live in registers, no per-row array is indexed dynamically (no scratch memory).  The column sums go
// wave butterfly -> LDS -> one partial row per 256-row chunk; the finish pass adds the chunks in order.  No float atomics: every
// sum has a fixed order, two runs give the same bits.  Inputs and outputs are f32; the arithmetic in between is f64 (a row is 2E
// values and a handful of exp / log1p / erf: the launches stay bound by their loads and stores), so every output is the correctly
// rounded f32 of its formula up to the f64 rounding -- cv2's cancelling sums included -- and v_k / v_{k+1} are kept as f64.  Forward
// and backward evaluate sigma and noisy with the same instructions (ng_noisy), so the backward's `noisy > v_{k+1}` compare decides
// exactly as the forward's did.
#include "smoe_common.h"

namespace {

constexpr int NG_THREADS = 256;                   // rows per workgroup = rows per chunk of the column partials
constexpr int NG_WAVES = NG_THREADS / 64;
constexpr int NG_MAX_E = 32;
constexpr int NG_MAX_K = 4;
constexpr int NG_SLOTS = NG_MAX_K + 1;            // the k + 1 best of a row
constexpr double NG_NOISE_EPS = 1e-2;

// torch's softplus (beta 1, threshold 20) + noise_epsilon
__device__ __forceinline__ double ng_sigma(double raw) { return (raw > 20.0 ? raw : log1p(exp(raw))) + NG_NOISE_EPS; }
// softplus'(raw) = sigmoid(raw); 1 on the linear branch
__device__ __forceinline__ double ng_dsoftplus(double raw) { return raw > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-raw)); }
// noisy value of one expert of a row (eval: the clean logit)
__device__ __forceinline__ double ng_noisy(const float* __restrict__ l, const float* __restrict__ ep, int E, int e, int training) {
  const double c = l[e];
  return training ? fma(ep ? (double)ep[e] : 0.0, ng_sigma(l[E + e]), c) : c;
}

// ---- forward, row pass ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NG_THREADS) void noisy_gate_rows_kernel(const float* __restrict__ logits2, const float* __restrict__ eps,
                                                                     int64_t T, int E, int k, int training, int64_t* __restrict__ idx,
                                                                     float* __restrict__ score, double* __restrict__ keep,
                                                                     int32_t* __restrict__ next, double* __restrict__ partial) {
  __shared__ double red[NG_WAVES][2 * NG_MAX_E];  // per wave: [E] importance, [E] load
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t t = (int64_t)blockIdx.x * NG_THREADS + tid;
  const bool valid = t < T;
  const float* l = logits2 + (valid ? t : 0) * 2 * E;
  const float* ep = eps ? eps + (valid ? t : 0) * E : nullptr;

  // the k + 1 best: slot j starts as (-inf, expert j) so that a row of NaNs still names experts inside [0, E)
  double v[NG_SLOTS];
  int id[NG_SLOTS];
#pragma unroll
  for (int j = 0; j < NG_SLOTS; ++j) {
    v[j] = -INFINITY;
    id[j] = j < E ? j : E - 1;
  }
  if (valid) {
    for (int e = 0; e < E; ++e) {
      const double n = ng_noisy(l, ep, E, e, training);
      // strict compares: an equal value stays behind the one that came first (the lower expert id)
      if (n > v[NG_SLOTS - 1]) {
        v[NG_SLOTS - 1] = n;
        id[NG_SLOTS - 1] = e;
#pragma unroll
        for (int j = NG_SLOTS - 1; j >= 1; --j) {
          if (v[j] > v[j - 1]) {
            const double tv = v[j]; v[j] = v[j - 1]; v[j - 1] = tv;
            const int ti = id[j]; id[j] = id[j - 1]; id[j - 1] = ti;
          }
        }
      }
    }
  }
  // score = softmax over the k kept; v_k, v_{k+1} and the (k + 1)-th expert are what the backward keeps
  double s[NG_MAX_K];
  double ssum = 0.0, vk = 0.0, vk1 = 0.0;
  int inext = 0;
#pragma unroll
  for (int j = 0; j < NG_MAX_K; ++j) {
    s[j] = j < k ? exp(v[j] - v[0]) : 0.0;
    ssum += s[j];
  }
  const double inv = 1.0 / ssum;
#pragma unroll
  for (int j = 0; j < NG_SLOTS; ++j) {
    if (j == k - 1) vk = v[j];
    if (j == k) { vk1 = v[j]; inext = id[j]; }
  }
#pragma unroll
  for (int j = 0; j < NG_MAX_K; ++j) {
    s[j] *= inv;
    if (valid && j < k) {
      idx[t * k + j] = id[j];
      score[t * k + j] = (float)s[j];
    }
  }
  if (valid) {
    keep[2 * t] = vk;
    keep[2 * t + 1] = vk1;
    next[t] = inext;
  }
  // column sums of this chunk: importance (the scores at their experts) and load (P[t, e], training only)
  for (int e = 0; e < E; ++e) {
    double ci = 0.0, cl = 0.0;
    if (valid) {
#pragma unroll
      for (int j = 0; j < NG_MAX_K; ++j) ci += (j < k && id[j] == e) ? s[j] : 0.0;
      if (training) {
        const double c = l[e], sg = ng_sigma(l[E + e]);
        const double n = fma(ep ? (double)ep[e] : 0.0, sg, c);
        const double thr = n > vk1 ? vk1 : vk;
        cl = 0.5 * (1.0 + erf((c - thr) / sg * 0.70710678118654752440));
      }
    }
    ci = wave_sum(ci);
    cl = wave_sum(cl);
    if (lane == 0) {
      red[wave][e] = ci;
      red[wave][E + e] = cl;
    }
  }
  __syncthreads();
  if (tid < 2 * E) {
    double a = red[0][tid];
#pragma unroll
    for (int w = 1; w < NG_WAVES; ++w) a += red[w][tid];
    partial[(int64_t)blockIdx.x * 2 * E + tid] = a;
  }
}

// ---- forward, finish pass -----------------------------------------------------------------------------------------------------------
// thread c < 2 E adds column c of the chunk partials in chunk order; then cv2(v) = var_unbiased(v) / (mean(v)^2 + 1e-10) of both
// vectors and d cv2 / d v_e = (2 (v_e - mean) / (E - 1) (mean^2 + 1e-10) - var 2 mean / E) / (mean^2 + 1e-10)^2
__global__ __launch_bounds__(64) void noisy_gate_finish_kernel(const double* __restrict__ partial, int n_chunks, int E,
                                                               float* __restrict__ imp, float* __restrict__ load,
                                                               float* __restrict__ aux, float* __restrict__ coef_imp,
                                                               float* __restrict__ coef_load) {
  __shared__ double col[2 * NG_MAX_E];
  __shared__ double cv[2];
  const int c = threadIdx.x;
  if (c < 2 * E) {
    double a = 0.0;
    for (int q = 0; q < n_chunks; ++q) a += partial[(int64_t)q * 2 * E + c];
    col[c] = a;
  }
  __syncthreads();
  if (c < 2 * E) {
    const int which = c / E, e = c - which * E;
    const double* vec = col + which * E;
    double sum = 0.0;
    for (int q = 0; q < E; ++q) sum += vec[q];
    const double mean = sum / (double)E;
    double ss = 0.0;
    for (int q = 0; q < E; ++q) ss += (vec[q] - mean) * (vec[q] - mean);
    const double var = ss / (double)(E - 1);
    const double den = mean * mean + 1e-10;
    const double dv = (2.0 * (vec[e] - mean) / (double)(E - 1) * den - var * (2.0 * mean / (double)E)) / (den * den);
    (which ? load : imp)[e] = (float)vec[e];
    (which ? coef_load : coef_imp)[e] = (float)dv;
    if (e == 0) cv[which] = var / den;
  }
  __syncthreads();
  if (c == 0) *aux = (float)(cv[0] + cv[1]);
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
// s_j = softmax over the k kept noisy values, recomputed;  g_j = dscore_j + cs cI[i_j];  dn[i_j] = s_j (g_j - sum_i s_i g_i)
// a_e = cs cL[e] phi(z_e) / sigma_e, z_e = (clean_e - thr_e) / sigma_e:  dclean_e += a_e,  dsigma_e -= a_e z_e,
//   dn[thr's expert] -= a_e   (thr_e = v_{k+1} -> expert i_{k+1} where noisy_e > v_{k+1}, else v_k -> expert i_k)
// dclean += dn, dsigma += dn eps, draw = dsigma softplus'(raw).  cs = *coef_scale; without it the loss terms are left out.
__global__ __launch_bounds__(NG_THREADS) void noisy_gate_bwd_kernel(const float* __restrict__ logits2, const float* __restrict__ eps,
                                                                    const int64_t* __restrict__ idx, const double* __restrict__ keep,
                                                                    const int32_t* __restrict__ next, const float* __restrict__ dscore,
                                                                    const float* __restrict__ coef_imp,
                                                                    const float* __restrict__ coef_load,
                                                                    const float* __restrict__ coef_scale, int64_t T, int E, int k,
                                                                    int training, float* __restrict__ dlogits2) {
  const int64_t t = (int64_t)blockIdx.x * NG_THREADS + threadIdx.x;
  if (t >= T) return;
  const float* l = logits2 + t * 2 * E;
  const float* ep = eps ? eps + t * E : nullptr;
  float* o = dlogits2 + t * 2 * E;
  const bool with_loss = coef_scale != nullptr;
  const double cs = with_loss ? (double)*coef_scale : 0.0;
  int ij[NG_MAX_K];
  double s[NG_MAX_K], g[NG_MAX_K];
  double n0 = 0.0, ssum = 0.0;
#pragma unroll
  for (int j = 0; j < NG_MAX_K; ++j) {
    ij[j] = -1; s[j] = 0.0; g[j] = 0.0;
    if (j < k) {
      const int64_t e = idx[t * k + j];
      ij[j] = (e >= 0 && e < E) ? (int)e : -1;
      if (ij[j] >= 0) {
        const double n = ng_noisy(l, ep, E, ij[j], training);
        if (j == 0) n0 = n;
        s[j] = exp(n - n0);
        ssum += s[j];
        g[j] = dscore ? (double)dscore[t * k + j] : 0.0;
        if (with_loss) g[j] = fma(cs, (double)coef_imp[ij[j]], g[j]);
      }
    }
  }
  const double inv = 1.0 / ssum;
  double inner = 0.0;
  int ik = -1;
#pragma unroll
  for (int j = 0; j < NG_MAX_K; ++j) {
    s[j] *= inv;
    inner = fma(s[j], g[j], inner);
    if (j == k - 1) ik = ij[j];
  }
#pragma unroll
  for (int j = 0; j < NG_MAX_K; ++j) g[j] = s[j] * (g[j] - inner);      // dn of the j-th kept expert
  const bool with_load = with_loss && training;
  const double vk = keep[2 * t], vk1 = keep[2 * t + 1];
  double sum_in = 0.0, sum_out = 0.0;
  for (int e = 0; e < E; ++e) {
    double dn = 0.0;
#pragma unroll
    for (int j = 0; j < NG_MAX_K; ++j) dn += (ij[j] == e) ? g[j] : 0.0;
    const double epe = ep ? (double)ep[e] : 0.0;
    double dclean = dn, draw = 0.0;
    if (training) {
      const double raw = l[E + e];
      double dsig = dn * epe;
      if (with_load) {
        const double c = l[e], sg = ng_sigma(raw);
        const double n = fma(epe, sg, c);
        const bool in = n > vk1;
        const double z = (c - (in ? vk1 : vk)) / sg;
        const double a = cs * (double)coef_load[e] * (0.39894228040143267794 * exp(-0.5 * z * z)) / sg;
        dclean += a;
        dsig = fma(-a, z, dsig);
        if (in) sum_in += a; else sum_out += a;
      }
      draw = dsig * ng_dsoftplus(raw);
    }
    if (with_load && (e == ik || e == next[t])) continue;      // the thresholds' own experts: written below, once the sums are known
    o[e] = (float)dclean;
    o[E + e] = (float)draw;
  }
  if (with_load) {                                // dn of a threshold's expert -= the sum of the a_e that read that threshold
    const int in_e = next[t];
#pragma unroll 1
    for (int q = 0; q < 2; ++q) {
      const int e = q ? in_e : ik;
      if (e < 0 || e >= E || (q && e == ik)) continue;
      double dn = 0.0;
#pragma unroll
      for (int j = 0; j < NG_MAX_K; ++j) dn += (ij[j] == e) ? g[j] : 0.0;
      dn -= (e == ik ? sum_out : 0.0) + (e == in_e ? sum_in : 0.0);
      const double c = l[e], raw = l[E + e], epe = ep ? (double)ep[e] : 0.0, sg = ng_sigma(raw);
      const double n = fma(epe, sg, c);
      const bool in = n > vk1;
      const double z = (c - (in ? vk1 : vk)) / sg;
      const double a = cs * (double)coef_load[e] * (0.39894228040143267794 * exp(-0.5 * z * z)) / sg;
      o[e] = (float)(dn + a);
      o[E + e] = (float)(fma(-a, z, dn * epe) * ng_dsoftplus(raw));
    }
  }
}

inline int64_t ng_chunks(int64_t T) { return (T + NG_THREADS - 1) / NG_THREADS; }

int ng_check_sizes(const char* who, int64_t T, int E, int k) {
  SMOE_REQUIRE(E >= 2 && E <= NG_MAX_E, "%s: E=%d out of range [2, %d]", who, E, NG_MAX_E);
  SMOE_REQUIRE(k >= 1 && k <= NG_MAX_K && k < E, "%s: k=%d out of range (1 <= k <= %d, k < E=%d: the load needs a (k+1)-th value)", who, k,
               NG_MAX_K, E);
  SMOE_REQUIRE(T >= 0 && ng_chunks(T) <= (1 << 24), "%s: T=%lld out of range", who, (long long)T);
  return 0;
}

}  // namespace

// workspace: [chunks x 2E f64: importance | load column sums per 256-row chunk]
extern "C" size_t smoe_noisy_gate_workspace_bytes(int64_t T, int E) {
  if (T < 0 || E < 1) return 0;
  return (size_t)(ng_chunks(T) + 1) * 2 * (size_t)E * 8;
}

extern "C" int smoe_noisy_gate_fwd(const float* logits2, const float* eps, int64_t T, int E, int k, int training, int64_t* idx,
                                   float* score, double* keep, int32_t* next, float* imp, float* load, float* aux, float* coef_imp,
                                   float* coef_load, void* workspace, size_t workspace_bytes, void* stream) {
  if (ng_check_sizes("smoe_noisy_gate_fwd", T, E, k)) return 1;
  SMOE_REQUIRE(imp && load && aux && coef_imp && coef_load && (T == 0 || (logits2 && idx && score && keep && next)),
               "smoe_noisy_gate_fwd: null pointer");
  SMOE_REQUIRE(workspace && workspace_bytes >= smoe_noisy_gate_workspace_bytes(T, E), "smoe_noisy_gate_fwd: workspace too small (%zu < %zu)",
               workspace_bytes, smoe_noisy_gate_workspace_bytes(T, E));
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunks = ng_chunks(T);
  double* partial = reinterpret_cast<double*>(workspace);
  if (chunks > 0) {
    hipLaunchKernelGGL(noisy_gate_rows_kernel, dim3((unsigned)chunks), dim3(NG_THREADS), 0, s, logits2, eps, T, E, k, training ? 1 : 0, idx,
                       score, keep, next, partial);
    SMOE_CHECK_LAUNCH("smoe_noisy_gate_fwd/rows");
  }
  hipLaunchKernelGGL(noisy_gate_finish_kernel, dim3(1), dim3(64), 0, s, partial, (int)chunks, E, imp, load, aux, coef_imp, coef_load);
  SMOE_CHECK_LAUNCH("smoe_noisy_gate_fwd/finish");
  return 0;
}

extern "C" int smoe_noisy_gate_bwd(const float* logits2, const float* eps, const int64_t* idx, const double* keep, const int32_t* next,
                                   const float* dscore, const float* coef_imp, const float* coef_load,
                                   const float* coef_scale, int64_t T, int E, int k, int training, float* dlogits2, void* stream) {
  if (ng_check_sizes("smoe_noisy_gate_bwd", T, E, k)) return 1;
  if (T == 0) return 0;
  SMOE_REQUIRE(logits2 && idx && keep && next && dlogits2, "smoe_noisy_gate_bwd: null pointer");
  SMOE_REQUIRE(!coef_scale || (coef_imp && coef_load), "smoe_noisy_gate_bwd: coef_scale without the coefficient vectors");
  hipLaunchKernelGGL(noisy_gate_bwd_kernel, dim3((unsigned)ng_chunks(T)), dim3(NG_THREADS), 0, (hipStream_t)stream, logits2, eps, idx,
                     keep, next, dscore, coef_imp, coef_load, coef_scale, T, E, k, training ? 1 : 0, dlogits2);
  SMOE_CHECK_LAUNCH("smoe_noisy_gate_bwd");
  return 0;
}
