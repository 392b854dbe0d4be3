// Router, 16-lanes-per-token layout (E <= 8 at d in {192, 384, 768, 1024}; E <= 32 at d in {768, 1024}): the fast
// path of smoe_router_topk, the fused LayerNorm + router, and the LayerNorm kernel.  The kernel template lives in
// router16_kernel.h (shared with gate.hip, which instantiates the token-skip-gate variants).
#include "router_launch.h"
#include "router_mt_kernel.h"
#include <cstdlib>

namespace {
using namespace r16;

// LayerNorm alone, same 16-lanes-per-token layout and arithmetic as the fused router (block glue for the
// attention half of the block: `attn(norm1(x))`, models/vision_transformer.py:320): one pass, 16-bit or f32 output.
template <typename XT, int NJ, typename OT>
__global__ __launch_bounds__(R16_THREADS, 4) void layernorm16_kernel(const XT* __restrict__ x, const float* __restrict__ g,
                                                                     const float* __restrict__ b, float eps, int64_t T,
                                                                     int d, OT* __restrict__ out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, u = lane & 15;
  const int nchunk = d >> 2;
  const int64_t slot_gid = ((int64_t)blockIdx.x * (R16_THREADS / 64) + wave) * 4 + q;
  const int64_t slot_stride = (int64_t)gridDim.x * (R16_THREADS / 64) * 4;
  for (int64_t it0 = slot_gid - q; it0 < T; it0 += slot_stride) {
    const int64_t t = it0 + q;
    const bool live = t < T;
    float xv[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = u + 16 * j;
      if (live && c < nchunk) load4(x + t * (int64_t)d + c * 4, xv[j]);
      else xv[j][0] = xv[j][1] = xv[j][2] = xv[j][3] = 0.f;
    }
    float s1 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) s1 += (xv[j][0] + xv[j][1]) + (xv[j][2] + xv[j][3]);
    const float mean = row16_sum(s1) / (float)d;
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = u + 16 * j;
      if (c < nchunk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float dv = xv[j][i] - mean; s2 = fmaf(dv, dv, s2); }
      }
    }
    const float rstd = rsqrtf(row16_sum(s2) / (float)d + eps);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = u + 16 * j;
      if (live && c < nchunk) {
        // gamma / beta come from L1/L2 at use (6 KB, shared by every wave): holding them in registers would cost
        // 96 VGPRs and spill
        const f32x4 gg = g ? *reinterpret_cast<const f32x4*>(g + c * 4) : f32x4{1.f, 1.f, 1.f, 1.f};
        const f32x4 bb = b ? *reinterpret_cast<const f32x4*>(b + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = fmaf((xv[j][i] - mean) * rstd, gg[i], bb[i]);
        OT* dst = out + t * (int64_t)d + c * 4;
        if constexpr (std::is_same<OT, float>::value) {
          *reinterpret_cast<f32x4*>(dst) = f32x4{o[0], o[1], o[2], o[3]};
        } else if constexpr (std::is_same<OT, f16>::value) {
          f16x4 v; v[0] = (f16)o[0]; v[1] = (f16)o[1]; v[2] = (f16)o[2]; v[3] = (f16)o[3];
          *reinterpret_cast<f16x4*>(dst) = v;
        } else {
          s16x4 v; v[0] = (short)f32_to_bf16(o[0]); v[1] = (short)f32_to_bf16(o[1]); v[2] = (short)f32_to_bf16(o[2]); v[3] = (short)f32_to_bf16(o[3]);
          *reinterpret_cast<s16x4*>(dst) = v;
        }
      }
    }
  }
}

// LayerNorm alone, ONE WAVE PER ROW (lane l holds the elements [8 l + 512 i, 8 l + 512 i + 8) of the row: whole 32-byte pieces,
// two-pass statistics over the wave).  Same arithmetic order inside a lane's pieces as the 16-lanes-per-token kernel? No -- the
// reduction tree differs, so the two kernels agree to f32 rounding, not bit for bit; a shape uses ONE of them, always (below).
// At d = 1024 the 16-lane layout holds 64 row elements per lane and reaches 3.1 TB/s (cfg 4's model: 72.6 us for 227 MB,
// profiles/r05_cfg4_kernel_stats.csv); a wave per row holds 16.
template <typename XT, int NI, typename OT>
__global__ __launch_bounds__(256) void layernorm_wave_kernel(const XT* __restrict__ x, const float* __restrict__ g,
                                                             const float* __restrict__ b, float eps, int64_t T, int d,
                                                             OT* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave_gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t t = wave_gid; t < T; t += nwaves) {
    float v[NI][8];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int c = lane * 8 + 512 * i;
      if (c < d) load8(x + t * (int64_t)d + c, v[i]);
      else {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[i][q] = 0.f;
      }
    }
    float mean, rstd;
    wave_row_stats<NI>(v, d, lane, eps, mean, rstd);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int c = lane * 8 + 512 * i;
      if (c < d) {
        float gg[8], bb[8], o[8];
        if (g) load8(g + c, gg);
        if (b) load8(b + c, bb);
#pragma unroll
        for (int q = 0; q < 8; ++q) o[q] = wave_row_affine(v[i][q], mean, rstd, g ? gg[q] : 1.f, b ? bb[q] : 0.f);
        store8(out + t * (int64_t)d + c, o);
      }
    }
  }
}

template <typename XT, typename OT>
int ln_dispatch_nj(const void* x, const float* g, const float* b, float eps, int64_t T, int d, void* out, hipStream_t s) {
  if (smoe_ln_wave_layout(d) && d % 8 == 0 && d <= 1024) {
    int64_t blocks = (T + 3) / 4;
    const int wg = (int)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks));
    if (d <= 512) hipLaunchKernelGGL((layernorm_wave_kernel<XT, 1, OT>), dim3(wg), dim3(256), 0, s, (const XT*)x, g, b, eps, T, d, (OT*)out);
    else hipLaunchKernelGGL((layernorm_wave_kernel<XT, 2, OT>), dim3(wg), dim3(256), 0, s, (const XT*)x, g, b, eps, T, d, (OT*)out);
    SMOE_CHECK_LAUNCH("smoe_layernorm/wave");
    return 0;
  }
  // one 16-token group per workgroup (no loop): the dispatcher back-fills CUs as groups retire, so there is no
  // 1-vs-2-iteration imbalance between resident workgroups
  int64_t need = (T + 15) / 16;
  const int grid = (int)(need < 1 ? 1 : (need > (1 << 20) ? (1 << 20) : need));
#define LN_LAUNCH(NJ) hipLaunchKernelGGL((layernorm16_kernel<XT, NJ, OT>), dim3(grid), dim3(R16_THREADS), 0, s, (const XT*)x, g, b, eps, T, d, (OT*)out)
  switch (d) {
    case 192: LN_LAUNCH(3); break;
    case 384: LN_LAUNCH(6); break;
    case 768: LN_LAUNCH(12); break;
    case 1024: LN_LAUNCH(16); break;
    default: smoe_set_error("smoe_layernorm: unsupported d=%d", d); return 1;
  }
#undef LN_LAUNCH
  SMOE_CHECK_LAUNCH("smoe_layernorm");
  return 0;
}

template <typename XT, int NJ, bool LN, typename NT, int EB> int launch16(const RouterArgs& a) {
  // 32 experts: the f32 weight image (96-128 KB) leaves room for ONE workgroup per CU; 512 threads put 8 waves behind it
  // instead of 4 (the f32 pass only: the f64 passes would spill at that size, and the redo pass handles a handful of tokens)
  constexpr int NTH = EB > 16 ? 512 : R16_THREADS;
  const size_t smem = router16_smem<NJ, LN, EB, 0>();
  const int64_t tok_per_block = (NTH / 64) * 4;  // (of the f32 pass; historical: it also sizes the 256-thread f64 passes' grid)
  int64_t need = (a.T + tok_per_block - 1) / tok_per_block;
  // <= 768 workgroups (3 resident per CU; 512 = 2 per CU for the 16-expert image: the LDS weight image is loaded once
  // per workgroup), every workgroup the same number of 16-token groups
  constexpr int64_t max_wg = EB <= 8 ? 768 : (EB <= 16 ? 512 : 256);
  const int64_t iters = (need + max_wg - 1) / max_wg;
  const int grid = (int)(need < 1 ? 1 : (need + iters - 1) / (iters < 1 ? 1 : iters));
  // with a chunk histogram every workgroup of the f32 pass walks ONE contiguous chunk of R16_HIST_TOK tokens; an all-f64 run
  // writes none (its f32 pass decides nothing), so it keeps the plain grid
  const HistArgs ha{(EB == 8 && !a.all_f64) ? a.hist : nullptr, R16_HIST_TOK};
  const int grid0 = ha.hist ? (int)((a.T + R16_HIST_TOK - 1) / R16_HIST_TOK) : grid;
  const RouterPlan plan{grid0, grid, 16, LN, "smoe_router_topk/f32", "smoe_router_topk/f64", "smoe_router_topk/redo"};
  if (smem > 64 * 1024) {  // 16 experts x d 1024 (+ LayerNorm vectors): above the default dynamic-LDS limit
    SMOE_ENSURE_SMEM(router16_kernel<XT, NJ, 0, LN, NT, EB, 0, NTH>);
    SMOE_ENSURE_SMEM(router16_kernel<XT, NJ, 1, LN, NT, EB, 0, R16_THREADS>);
  }
#define R16_LAUNCH(MODE, THREADS, g, rc, rl)                                                                                 \
  hipLaunchKernelGGL((router16_kernel<XT, NJ, MODE, LN, NT, EB, 0, THREADS>), dim3(g), dim3(THREADS), smem, a.stream,        \
                     (const XT*)a.x, a.ln_g, a.ln_b, a.ln_eps, (NT*)a.xn16, a.xn32, a.wg, a.bg, a.noise, a.T, a.d, a.E, a.k, \
                     a.gate_kind, rc, rl, a.idx, a.score, a.logits, a.probs, a.gate, ha)
  return run_router_passes(
      a, plan, [&](int g, int32_t* rc, int32_t* rl) { R16_LAUNCH(0, NTH, g, rc, rl); },
      [&](int g, int32_t* rc, int32_t* rl) { R16_LAUNCH(1, R16_THREADS, g, rc, rl); });
#undef R16_LAUNCH
}

// 16 / 32 experts on the f32 matrix cores (router_mt_kernel.h); SMOE_ROUTER_MT=0 keeps the 16-lanes-per-token kernel (A/B)
static bool use_router_mt() {
  static const bool on = [] { const char* v = getenv("SMOE_ROUTER_MT"); return !(v && v[0] == '0'); }();
  return on;
}
// SMOE_ROUTER_MT_HALVES=1 = the one-half form of the matrix-core f32 pass (A/B)
static bool want_two_halves() {
  static const bool on = [] { const char* v = getenv("SMOE_ROUTER_MT_HALVES"); return !(v && v[0] == '1'); }();
  return on;
}

template <typename XT, int MP, bool LN, typename NT, int EB> int launch_mt(const RouterArgs& a) {
  using namespace rmt;
  constexpr size_t smem = router_mt_smem<MP, LN, EB, 1>();
  static_assert(smem <= 160 * 1024, "router_mt: LDS image too large");
  // An image that leaves room for ONE workgroup per CU (E = 32) runs the f32 pass on TWO four-wave halves per workgroup (HV = 2:
  // two waves per SIMD on the same image; router_mt_kernel.h) when both halves' exchange areas fit.  The f64 passes always run
  // one half.
  constexpr bool can2 = 2 * smem > 160 * 1024 && router_mt_smem<MP, LN, EB, 2>() <= 160 * 1024;
  const bool two = can2 && want_two_halves();
  const int64_t n_tiles = (a.T + 15) / 16;
  const int per_cu = (int)((160 * 1024) / smem) < 1 ? 1 : (int)((160 * 1024) / smem);
  // every workgroup the same number of tiles (the weight image is staged once per workgroup): `work` items over at most max_wg
  auto even_grid = [](int64_t work, int64_t max_wg) {
    const int64_t iters = (work + max_wg - 1) / max_wg;
    return (int)(work < 1 ? 1 : (work + iters - 1) / (iters < 1 ? 1 : iters));
  };
  const int grid = even_grid(n_tiles, (int64_t)smoe_num_cus() * (per_cu > 2 ? 2 : per_cu));
  // the f32 pass on two halves: half as many workgroups, each walking the tiles of two
  const int grid_f32 = two ? even_grid((n_tiles + 1) / 2, smoe_num_cus()) : grid;
  const RouterPlan plan{grid_f32, grid, 16, LN, "smoe_router_topk/mt f32", "smoe_router_topk/mt f64", "smoe_router_topk/mt redo"};
  // always registered (historical: launch16 / launch_gate register above 64 KiB only; smoe_init pre-sets exactly this set)
  SMOE_ENSURE_SMEM(router_mt_kernel<XT, MP, 0, LN, NT, EB>);
  SMOE_ENSURE_SMEM(router_mt_kernel<XT, MP, 1, LN, NT, EB>);
  if constexpr (can2) SMOE_ENSURE_SMEM(router_mt_kernel<XT, MP, 0, LN, NT, EB, 2>);
#define MT_LAUNCH(MODE, HV, SMEM, g, rc, rl)                                                                                  \
  hipLaunchKernelGGL((router_mt_kernel<XT, MP, MODE, LN, NT, EB, HV>), dim3(g), dim3(HV * MT_THREADS), SMEM, a.stream,        \
                     (const XT*)a.x, a.ln_g, a.ln_b, a.ln_eps, (NT*)a.xn16, a.xn32, a.wg, a.bg, a.noise, a.T, a.E, a.k,       \
                     a.gate_kind, rc, rl, a.idx, a.score, a.logits, a.probs)
  return run_router_passes(
      a, plan,
      [&](int g, int32_t* rc, int32_t* rl) {
        if constexpr (can2) {
          if (two) {
            MT_LAUNCH(0, 2, (router_mt_smem<MP, LN, EB, 2>()), g, rc, rl);
            return;
          }
        }
        MT_LAUNCH(0, 1, smem, g, rc, rl);
      },
      [&](int g, int32_t* rc, int32_t* rl) { MT_LAUNCH(1, 1, smem, g, rc, rl); });
#undef MT_LAUNCH
}

// -1 when the shape has no instantiation here
template <typename XT, bool LN, typename NT> int dispatch16(const RouterArgs& a) {
  const int d = a.d, E = a.E;
#define R16_BY_D(LAUNCH, N768, N1024, EB)                   \
  switch (d) {                                              \
    case 768: return LAUNCH<XT, N768, LN, NT, EB>(a);       \
    case 1024: return LAUNCH<XT, N1024, LN, NT, EB>(a);     \
  }                                                         \
  return -1
  if (E > 8 && use_router_mt()) {
    if (E > 16) { R16_BY_D(launch_mt, 6, 8, 32); }
    R16_BY_D(launch_mt, 6, 8, 16);
  }
  // 32 experts per lane: one workgroup per CU (the f32 weight image is 96-128 KB); 16 / 32 experts are instantiated for the
  // ViT-B / ViT-L widths only (compile time)
  if (E > 16) { R16_BY_D(launch16, 12, 16, 32); }
  if (E > 8) { R16_BY_D(launch16, 12, 16, 16); }
  switch (d) {
    case 192: return launch16<XT, 3, LN, NT, 8>(a);
    case 384: return launch16<XT, 6, LN, NT, 8>(a);
  }
  R16_BY_D(launch16, 12, 16, 8);
#undef R16_BY_D
}

// LayerNorm off: NT is not looked at, one instantiation (f16) serves
template <typename XT> int dispatch16_ln(const RouterArgs& a) {
  if (!a.ln_on) return dispatch16<XT, false, f16>(a);
  if (a.xn16_dtype == SMOE_BF16) return dispatch16<XT, true, bf16_bits>(a);
  return dispatch16<XT, true, f16>(a);
}

}  // namespace

static bool shape_ok16(int d, int E, int k) {
  if (k > R16_MAX_K) return false;
  if (E <= 8) return d == 192 || d == 384 || d == 768 || d == 1024;
  return E <= 32 && (d == 768 || d == 1024);
}

// returns -1 when the shape is not covered by this fast path (caller falls back to router.hip)
int smoe_router16_try(const RouterArgs& a) {
  if (!shape_ok16(a.d, a.E, a.k)) return -1;
  return router_by_x_dtype(a, [&](auto xt) { return dispatch16_ln<decltype(xt)>(a); });
}

extern "C" int smoe_ln_router_supported(int d, int E, int k) { return shape_ok16(d, E, k) ? 1 : 0; }

// Tokens per row of the chunk histogram that smoe_ln_router_topk / smoe_gate_ln_router write for this shape when the caller hands
// them a table (smoe_dispatch_plan_hist then needs no counting pass); 0 = this shape's router writes none.
extern "C" int smoe_router_chunk_hist_tokens(int d, int E, int k) {
  return (shape_ok16(d, E, k) && E <= 8 && k >= 1 && 1024 % (R16_HIST_TOK * k) == 0) ? R16_HIST_TOK : 0;
}

// LayerNorm + router in one pass over x (block glue fusion): xn = LN(x) * gamma + beta is
// written as the 16-bit operand image (xn16, f16 or bf16; may be NULL) and / or as f32 (xn32; may be NULL) and
// routed exactly like smoe_router_topk routes xn.  Shapes: smoe_ln_router_supported(d, E, k).
extern "C" int smoe_ln_router_topk(const void* x, int x_dtype, const float* ln_gamma, const float* ln_beta, float ln_eps,
                                   void* xn16, int xn16_dtype, float* xn32, const float* wg, const float* bg,
                                   const float* noise, int64_t T, int d, int E, int k, int gate_kind, int64_t* idx,
                                   float* score, float* logits_out, float* probs, int32_t* chunk_hist, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  RouterArgs a{};
  a.entry = "smoe_ln_router_topk";
  a.x = x, a.x_dtype = x_dtype;
  a.ln_on = true, a.ln_g = ln_gamma, a.ln_b = ln_beta, a.ln_eps = ln_eps, a.xn16 = xn16, a.xn16_dtype = xn16_dtype, a.xn32 = xn32;
  a.wg = wg, a.bg = bg, a.noise = noise;
  a.T = T, a.d = d, a.E = E, a.k = k;
  a.idx = idx, a.score = score, a.logits = logits_out, a.probs = probs;
  a.stream = (hipStream_t)stream;
  router_decode_gate_kind(a, gate_kind);
  if (T == 0) return 0;
  SMOE_REQUIRE(x && wg && idx && score, "smoe_ln_router_topk: null pointer");
  SMOE_REQUIRE(shape_ok16(d, E, k), "smoe_ln_router_topk: unsupported shape d=%d E=%d k=%d", d, E, k);
  SMOE_REQUIRE(T >= 0 && T < (1ll << 31), "smoe_ln_router_topk: bad T");
  SMOE_REQUIRE(k >= 1 && k <= E, "smoe_ln_router_topk: bad k");
  SMOE_REQUIRE(a.gate_kind == SMOE_GATE_NAIVE || (a.gate_kind == SMOE_GATE_SWITCH && k == 1), "smoe_ln_router_topk: bad gate");
  SMOE_REQUIRE(xn16_dtype == SMOE_F16 || xn16_dtype == SMOE_BF16, "smoe_ln_router_topk: xn16 must be f16 or bf16");
  if (int rc = router_take_workspace(a, workspace, workspace_bytes)) return rc;
  a.hist = (chunk_hist && smoe_router_chunk_hist_tokens(d, E, k)) ? chunk_hist : nullptr;
  return router_by_x_dtype(a, [&](auto xt) { return dispatch16_ln<decltype(xt)>(a); });
}

// LayerNorm over the last dimension, d in {192, 384, 768, 1024}; out dtype f32 / f16 / bf16.
extern "C" int smoe_layernorm(const void* x, int x_dtype, const float* gamma, const float* beta, float eps, int64_t T,
                              int d, void* out, int out_dtype, void* stream) {
  SMOE_REQUIRE(T >= 0 && (d == 192 || d == 384 || d == 768 || d == 1024), "smoe_layernorm: unsupported shape T=%lld d=%d", (long long)T, d);
  if (T == 0) return 0;
  SMOE_REQUIRE(x && out, "smoe_layernorm: null pointer");
  hipStream_t s = (hipStream_t)stream;
#define LN_OUT(XT)                                                                                   \
  switch (out_dtype) {                                                                               \
    case SMOE_F32: return ln_dispatch_nj<XT, float>(x, gamma, beta, eps, T, d, out, s);             \
    case SMOE_F16: return ln_dispatch_nj<XT, f16>(x, gamma, beta, eps, T, d, out, s);               \
    case SMOE_BF16: return ln_dispatch_nj<XT, bf16_bits>(x, gamma, beta, eps, T, d, out, s);        \
  }
  switch (x_dtype) {
    case SMOE_F32: LN_OUT(float) break;
    case SMOE_F16: LN_OUT(f16) break;
    case SMOE_BF16: LN_OUT(bf16_bits) break;
  }
#undef LN_OUT
  smoe_set_error("smoe_layernorm: bad dtype");
  return 1;
}
