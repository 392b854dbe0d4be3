// GShard gate (fmoe.gates.GShardGate; the rule is restated in INTEGRATION.md): the gate's own arithmetic behind the top-2 router.
//   smoe_gshard_prune     idx [T, 2] -> idx_out [T, 2]: per-expert capacity in FLAT order (entry i = 2 t + j is kept while fewer than
//                         `capacity` earlier entries named its expert), then random routing of the second choice (dropped when
//                         2 score[t, 1] < u[t]; it has still used its capacity slot); top1_counts[e] = #{t : idx[t, 0] == e}
//   smoe_gshard_aux       aux = mean_e(c_e m_e) num_expert^2, c_e = top1_counts[e] / T, m_e = mean_t softmax(logits[t, :])[e];
//                         coef[e] = d aux / d softmax(logits[t, :])[e] (any t)
//   smoe_gshard_gate_bwd  dlogits [T, E] of the balance loss and of score = softmax over the two kept logits, one pass
// Prune is two launches over n = 2 T flat entries in GS_CH-entry chunks: gshard_count (per-chunk LDS histograms of all entries and of
// the first choices) and gshard_rank, which sums the table rows in front of its own chunk (no scan launch), ranks its entries with
// wave ballots in flat order -- the ranking of dispatch.hip's plan_assign_kernel -- and writes idx_out.  Integer LDS atomics build
// histograms only; every rank and every float sum below has a fixed order: two runs give the same bits.
#include "smoe_common.h"

namespace {

constexpr int GS_THREADS = 256;
constexpr int GS_WAVES = GS_THREADS / 64;
constexpr int GS_ITERS = 4;                       // 64-entry steps per wave: a wave owns 256 consecutive entries
constexpr int GS_CH = GS_THREADS * GS_ITERS;      // entries per workgroup (512 tokens)
constexpr int GS_MAX_E = 256;
constexpr int64_t GS_MAX_TABLE = 1 << 20;         // chunks x E: every workgroup of gshard_rank walks the rows in front of its own

inline int64_t gs_nblk(int64_t n) { return n > 0 ? (n + GS_CH - 1) / GS_CH : 1; }

// ids outside [0, E) are dropped entries (-1), as the dispatch plan reads them
__device__ __forceinline__ int gs_id(const int64_t* __restrict__ idx, int64_t i, int64_t n, int E) {
  if (i >= n) return -1;
  const int64_t e = idx[i];
  return (e >= 0 && e < E) ? (int)e : -1;
}

__global__ __launch_bounds__(GS_THREADS) void gshard_count_kernel(const int64_t* __restrict__ idx, int64_t n, int E,
                                                                  int32_t* __restrict__ tab_all, int32_t* __restrict__ tab_top1) {
  __shared__ int32_t hist[2 * GS_MAX_E];          // [E] all entries, [E] first choices
  for (int e = threadIdx.x; e < 2 * E; e += GS_THREADS) hist[e] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * GS_CH;
#pragma unroll
  for (int it = 0; it < GS_ITERS; ++it) {
    const int64_t i = base + it * GS_THREADS + threadIdx.x;
    const int e = gs_id(idx, i, n, E);
    if (e >= 0) {
      atomicAdd(&hist[e], 1);
      if ((i & 1) == 0) atomicAdd(&hist[E + e], 1);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += GS_THREADS) {
    tab_all[(int64_t)blockIdx.x * E + e] = hist[e];
    tab_top1[(int64_t)blockIdx.x * E + e] = hist[E + e];
  }
}

// column sums of the rows [0, rows) of an i32 table [*, E] (E <= 256): thread (rr, e) adds the rows rr, rr + rpp, ...; thread e < E
// then adds the rpp partial sums in order.  Returns the sum in the threads tid < E.  (integers: any order gives the same value)
__device__ __forceinline__ int32_t gs_table_colsum(const int32_t* __restrict__ tab, int rows, int E, int32_t* red) {
  const int tid = threadIdx.x, rpp = GS_THREADS / E, rr = tid / E, e = tid - rr * E;
  int32_t acc = 0;
  if (rr < rpp)
    for (int b = rr; b < rows; b += rpp) acc += tab[(int64_t)b * E + e];
  __syncthreads();                                // (red may still be read from an earlier call)
  red[tid] = acc;
  __syncthreads();
  int32_t sum = 0;
  if (tid < E)
    for (int q = 0; q < rpp; ++q) sum += red[q * E + tid];
  return sum;
}

__global__ __launch_bounds__(GS_THREADS) void gshard_rank_kernel(
    const int64_t* __restrict__ idx, const float* __restrict__ score, const float* __restrict__ u, int64_t n, int E, int64_t capacity,
    const int32_t* __restrict__ tab_all, const int32_t* __restrict__ tab_top1, int nblk, int64_t* __restrict__ idx_out,
    int32_t* __restrict__ top1_counts) {
  __shared__ int32_t red[GS_THREADS];
  __shared__ int32_t run[GS_WAVES * GS_MAX_E];    // run[w][e]: raw rank of the next entry of expert e seen by wave w
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int me = (int)blockIdx.x;
  const int64_t wave_base = (int64_t)me * GS_CH + (int64_t)wave * (64 * GS_ITERS);

  for (int i = tid; i < GS_WAVES * E; i += GS_THREADS) run[i] = 0;
  if (me == 0) {                                  // (uniform over the workgroup)
    const int32_t c = gs_table_colsum(tab_top1, nblk, E, red);
    if (tid < E) top1_counts[tid] = c;
  }
  const int32_t base = gs_table_colsum(tab_all, me, E, red);   // entries of expert `tid` in front of this chunk
  // pass 1: per-wave histogram of its quarter
  int myidx[GS_ITERS];
#pragma unroll
  for (int it = 0; it < GS_ITERS; ++it) {
    const int e = gs_id(idx, wave_base + it * 64 + lane, n, E);
    myidx[it] = e;
    if (e >= 0) atomicAdd(&run[wave * E + e], 1);
  }
  __syncthreads();
  if (tid < E) {
    int32_t acc = base;
#pragma unroll
    for (int w = 0; w < GS_WAVES; ++w) {
      const int32_t c = run[w * E + tid];
      run[w * E + tid] = acc;
      acc += c;
    }
  }
  __syncthreads();
  // pass 2: in flat order inside the wave's quarter
  int32_t* myrun = run + wave * E;
#pragma unroll
  for (int it = 0; it < GS_ITERS; ++it) {
    const int64_t i = wave_base + it * 64 + lane;
    const int e = myidx[it];
    // rank among the lanes of this step with the same expert: peel one distinct expert per round
    int rank_in_step = 0, group = 0;
    unsigned long long todo = __ballot(e >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int e0 = __shfl(e, leader, 64);
      const unsigned long long m = __ballot(e == e0);
      if (e == e0) {
        rank_in_step = __popcll(m & ((1ull << lane) - 1ull));
        group = __popcll(m);
      }
      todo &= ~m;
    }
    if (i < n) {
      int64_t o = -1;
      if (e >= 0) {
        const int32_t raw = myrun[e] + rank_in_step;
        bool keep = capacity < 0 || (int64_t)raw < capacity;
        // random routing of the second choice, after the capacity (the slot stays used): an exact f32 compare (2 s is exact)
        if (keep && u && (i & 1)) keep = !(2.0f * score[i] < u[i >> 1]);
        o = keep ? (int64_t)e : -1;
      }
      idx_out[i] = o;
    }
    __builtin_amdgcn_wave_barrier();
    // the first lane of each expert group advances that expert's running rank
    if (e >= 0 && rank_in_step == 0) myrun[e] += group;
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- balance loss ---------------------------------------------------------------------------------------------------------------
// Column sums of softmax(logits) [T, E] per GA_ROWS-row chunk: thread r takes row r's max and 1 / sum(exp), then thread (row of the
// pass, column) adds p[r, e] over the chunk's rows (coalesced) and thread e adds the passes in order; one workgroup adds the chunks in
// order.  All f32, no float atomics.
constexpr int GA_ROWS = 256;

__global__ __launch_bounds__(256) void gshard_aux_partial_kernel(const float* __restrict__ logits, int64_t T, int E,
                                                                 float* __restrict__ partial) {
  __shared__ float smax[GA_ROWS], sinv[GA_ROWS], red[256];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * GA_ROWS;
  const int rows = (int)(T - r0 < GA_ROWS ? T - r0 : GA_ROWS);
  if (tid < rows) {
    const float* l = logits + (r0 + tid) * E;
    float m = l[0];
    for (int e = 1; e < E; ++e) m = fmaxf(m, l[e]);
    float s = 0.f;
    for (int e = 0; e < E; ++e) s += expf(l[e] - m);
    smax[tid] = m;
    sinv[tid] = 1.0f / s;
  }
  __syncthreads();
  const int rpp = 256 / E, rr = tid / E, e = tid - rr * E;
  float acc = 0.f;
  if (rr < rpp)
    for (int r = rr; r < rows; r += rpp) acc += expf(logits[(r0 + r) * E + e] - smax[r]) * sinv[r];
  red[tid] = acc;
  __syncthreads();
  if (tid < E) {
    float a = 0.f;
    for (int q = 0; q < rpp; ++q) a += red[q * E + tid];
    partial[(int64_t)blockIdx.x * E + tid] = a;
  }
}

__global__ __launch_bounds__(256) void gshard_aux_final_kernel(const float* __restrict__ partial, int n_chunks,
                                                               const int32_t* __restrict__ top1_counts, int64_t T, int E,
                                                               int num_expert, float* __restrict__ aux, float* __restrict__ coef) {
  __shared__ float term[GS_MAX_E];
  const int e = threadIdx.x;
  const float Tf = (float)(T < 1 ? 1 : T);
  const float scale = (float)num_expert * (float)num_expert / (float)E;
  if (e < E) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int c = 0;
    for (; c + 3 < n_chunks; c += 4) {
      a0 += partial[(int64_t)c * E + e];
      a1 += partial[(int64_t)(c + 1) * E + e];
      a2 += partial[(int64_t)(c + 2) * E + e];
      a3 += partial[(int64_t)(c + 3) * E + e];
    }
    for (; c < n_chunks; ++c) a0 += partial[(int64_t)c * E + e];
    const float ce = (float)top1_counts[e] / Tf;
    term[e] = ce * (((a0 + a1) + (a2 + a3)) / Tf);
    coef[e] = scale * ce / Tf;
  }
  __syncthreads();
  if (e == 0) {
    float acc = 0.f;
    for (int q = 0; q < E; ++q) acc += term[q];
    *aux = acc * scale;
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
// One thread per token; p = softmax(logits[t, :]) recomputed in f32 (the row is read three times from L1):
//   dl[t, e] = cs p[e] (coef[e] - sum_j p[j] coef[j])                            (balance loss; cs = *coef_scale)
//            + [e == idx[t, a]] s_a (ds_a - (s_0 ds_0 + s_1 ds_1))   a = 0, 1    (score = softmax over the two chosen logits)
// with ds_a = 0 for an entry the prune dropped (idx_out[t, a] < 0): the combine never read its score.
__global__ __launch_bounds__(256) void gshard_gate_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ idx,
                                                              const int64_t* __restrict__ idx_out, const float* __restrict__ score,
                                                              const float* __restrict__ dscore, const float* __restrict__ coef,
                                                              const float* __restrict__ coef_scale, int64_t T, int E,
                                                              float* __restrict__ dlogits) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const float* l = logits + t * E;
  float* o = dlogits + t * E;
  const int64_t i0 = idx[2 * t], i1 = idx[2 * t + 1];
  const float s0 = score[2 * t], s1 = score[2 * t + 1];
  const float ds0 = (dscore && idx_out[2 * t] >= 0) ? dscore[2 * t] : 0.f;
  const float ds1 = (dscore && idx_out[2 * t + 1] >= 0) ? dscore[2 * t + 1] : 0.f;
  const float inner = fmaf(s1, ds1, s0 * ds0);
  const float g0 = s0 * (ds0 - inner), g1 = s1 * (ds1 - inner);
  if (!coef) {
    for (int e = 0; e < E; ++e) o[e] = (e == i0 ? g0 : 0.f) + (e == i1 ? g1 : 0.f);
    return;
  }
  const float cs = coef_scale ? *coef_scale : 1.0f;
  float m = l[0];
  for (int e = 1; e < E; ++e) m = fmaxf(m, l[e]);
  float s = 0.f, dot = 0.f;
  for (int e = 0; e < E; ++e) {
    const float ex = expf(l[e] - m);
    s += ex;
    dot = fmaf(ex, coef[e], dot);
  }
  const float inv = 1.0f / s;
  dot *= inv;
  for (int e = 0; e < E; ++e) {
    const float p = expf(l[e] - m) * inv;
    o[e] = cs * (p * (coef[e] - dot)) + (e == i0 ? g0 : 0.f) + (e == i1 ? g1 : 0.f);
  }
}

}  // namespace

// workspace: [chunks x E i32: all entries][chunks x E i32: first choices]
extern "C" size_t smoe_gshard_prune_workspace_bytes(int64_t T, int E) {
  if (T < 0 || E < 1) return 0;
  return 2 * (size_t)gs_nblk(2 * T) * (size_t)E * 4;
}

extern "C" int smoe_gshard_prune(const int64_t* idx, const float* score, const float* u, int64_t T, int E, int64_t capacity,
                                 int64_t* idx_out, int32_t* top1_counts, void* workspace, size_t workspace_bytes, void* stream) {
  SMOE_REQUIRE(T >= 0 && T < (1ll << 30), "smoe_gshard_prune: T=%lld out of range", (long long)T);
  SMOE_REQUIRE(E >= 2 && E <= GS_MAX_E, "smoe_gshard_prune: E=%d out of range [2, %d] (top-2 needs two experts)", E, GS_MAX_E);
  const int64_t n = 2 * T, nblk = gs_nblk(n);
  SMOE_REQUIRE(nblk * E <= GS_MAX_TABLE, "smoe_gshard_prune: ceil(2 T / %d) * E = %lld exceeds %lld", GS_CH, (long long)(nblk * E),
               (long long)GS_MAX_TABLE);
  SMOE_REQUIRE(top1_counts && workspace && (T == 0 || (idx && idx_out)), "smoe_gshard_prune: null pointer");
  SMOE_REQUIRE(!u || T == 0 || score, "smoe_gshard_prune: random routing (u) needs the scores");
  SMOE_REQUIRE(workspace_bytes >= smoe_gshard_prune_workspace_bytes(T, E), "smoe_gshard_prune: workspace too small (%zu < %zu)",
               workspace_bytes, smoe_gshard_prune_workspace_bytes(T, E));
  hipStream_t s = (hipStream_t)stream;
  int32_t* tab_all = reinterpret_cast<int32_t*>(workspace);
  int32_t* tab_top1 = tab_all + nblk * E;
  hipLaunchKernelGGL(gshard_count_kernel, dim3((unsigned)nblk), dim3(GS_THREADS), 0, s, idx, n, E, tab_all, tab_top1);
  SMOE_CHECK_LAUNCH("smoe_gshard_prune/count");
  hipLaunchKernelGGL(gshard_rank_kernel, dim3((unsigned)nblk), dim3(GS_THREADS), 0, s, idx, score, u, n, E, capacity, tab_all, tab_top1,
                     (int)nblk, idx_out, top1_counts);
  SMOE_CHECK_LAUNCH("smoe_gshard_prune/rank");
  return 0;
}

extern "C" size_t smoe_gshard_aux_workspace_bytes(int64_t T, int E) {
  if (T < 0 || E < 1) return 0;
  return (size_t)((T + GA_ROWS - 1) / GA_ROWS + 1) * (size_t)E * 4;
}

extern "C" int smoe_gshard_aux(const float* logits, const int32_t* top1_counts, int64_t T, int E, int num_expert, float* aux,
                               float* coef, void* workspace, size_t workspace_bytes, void* stream) {
  SMOE_REQUIRE(T >= 0 && E >= 2 && E <= GS_MAX_E, "smoe_gshard_aux: bad sizes T=%lld E=%d (2 <= E <= %d)", (long long)T, E, GS_MAX_E);
  SMOE_REQUIRE(num_expert >= 1 && num_expert <= E && E % num_expert == 0,
               "smoe_gshard_aux: num_expert=%d must divide E=%d (E = num_expert x world size)", num_expert, E);
  SMOE_REQUIRE(top1_counts && aux && coef && (T == 0 || logits), "smoe_gshard_aux: null pointer");
  SMOE_REQUIRE(workspace && workspace_bytes >= smoe_gshard_aux_workspace_bytes(T, E), "smoe_gshard_aux: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunks = (T + GA_ROWS - 1) / GA_ROWS;
  SMOE_REQUIRE(chunks <= (1 << 24), "smoe_gshard_aux: too many rows");
  float* partial = reinterpret_cast<float*>(workspace);
  if (chunks > 0) {
    hipLaunchKernelGGL(gshard_aux_partial_kernel, dim3((unsigned)chunks), dim3(256), 0, s, logits, T, E, partial);
    SMOE_CHECK_LAUNCH("smoe_gshard_aux/partial");
  }
  hipLaunchKernelGGL(gshard_aux_final_kernel, dim3(1), dim3(256), 0, s, partial, (int)chunks, top1_counts, T, E, num_expert, aux, coef);
  SMOE_CHECK_LAUNCH("smoe_gshard_aux/final");
  return 0;
}

extern "C" int smoe_gshard_gate_bwd(const float* logits, const int64_t* idx, const int64_t* idx_out, const float* score,
                                    const float* dscore, const float* coef, const float* coef_scale, int64_t T, int E,
                                    float* dlogits, void* stream) {
  SMOE_REQUIRE(T >= 0 && E >= 2 && E <= GS_MAX_E, "smoe_gshard_gate_bwd: bad sizes T=%lld E=%d (2 <= E <= %d)", (long long)T, E, GS_MAX_E);
  SMOE_REQUIRE(T <= (int64_t)0x7fffffff * 256, "smoe_gshard_gate_bwd: too many rows");
  if (T == 0) return 0;
  SMOE_REQUIRE(logits && idx && idx_out && score && dlogits, "smoe_gshard_gate_bwd: null pointer");
  SMOE_REQUIRE(coef || !coef_scale, "smoe_gshard_gate_bwd: coef_scale without coef");
  hipLaunchKernelGGL(gshard_gate_bwd_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, idx, idx_out,
                     score, dscore, coef, coef_scale, T, E, dlogits);
  SMOE_CHECK_LAUNCH("smoe_gshard_gate_bwd");
  return 0;
}
