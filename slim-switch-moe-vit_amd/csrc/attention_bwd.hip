// Self-attention backward for ViT token counts (N <= 640, head dim 64): the training step's counterpart of attention.hip
// (models/vision_transformer.py:248-280 under engine.py:52-74's forward + backward).
//
//   S = scale q k^T,  P = softmax(S),  O = P v          (forward; P is never stored, only lse = log2 sum exp2(S log2 e))
//   dV = P^T dO,  dP = dO V^T,  dS = P (dP - delta) scale,  delta = rowsum(dO O),  dQ = dS K,  dK = dS^T Q
//
// N <= 256 (attn_bwd_kernel; 256 < N <= 640: the two kernels further down).
// One workgroup (4 waves, one per SIMD, up to 512 registers each) per (image, head); Q, K, V, dO of the head sit in LDS
// whole (row-major [token][64], 16-byte chunks XOR-swizzled: conflict-free ds_read_b128 row reads, 2-way transposed
// reads), queries are walked in steps of 32:
//   phase A  "key on the lane": wave w owns key tiles w, w + 4, ... and keeps their dK^T / dV^T ([64 x 16] each) in
//            accumulators over the whole sweep.  Per owned tile and step: S and dP as  A = Q / dO rows, B = K / V rows
//            (lane (g, key) ends up with queries 4 g + r), P = exp2(S c - lse), dS; then the accumulators of S / dP ARE
//            the B operands of  dV^T += dO^T P  and  dK^T += Q^T dS  (contraction over the 32 queries of the step; the
//            A operands are transposed reads of dO / Q) -- P never leaves the registers.
//   phase B  dQ contracts over KEYS, which sit on the lanes: dS (16 bit) crosses LDS once, as a [32 query][key] image;
//            wave w then computes  dQ^T[16 w .. 16 w + 15][32 queries] = K^T dS^T  over ALL keys (A = transposed reads
//            of K, B = row reads of the image), so dQ needs no reduction across waves or steps and is stored at once.
// Rows / keys >= N duplicate row N - 1 in LDS and carry P = dS = 0.  10 N^2 64 FLOP per (image, head) on the matrix cores.
#include "attention_tile.h"

namespace {

constexpr int DS_ROW = 512;                 // bytes per query row of the dS image (up to 256 keys x 2 B)
constexpr int DS_BYTES = 32 * DS_ROW;

// s + the dot product of two 8-element pieces, one fma chain in element order
template <typename HT> __device__ __forceinline__ float dot8(const u32x4& a, const u32x4& b, float s = 0.f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s = fmaf(from16<HT>((unsigned short)(a[e] & 0xffffu)), from16<HT>((unsigned short)(b[e] & 0xffffu)), s);
    s = fmaf(from16<HT>((unsigned short)(a[e] >> 16)), from16<HT>((unsigned short)(b[e] >> 16)), s);
  }
  return s;
}

template <typename HT, int NKT, int NW>
__global__ __launch_bounds__(64 * NW, 1) void attn_bwd_kernel(const HT* __restrict__ qkv, const HT* __restrict__ o,
                                                                 const HT* __restrict__ dout, const float* __restrict__ lse,
                                                                 HT* __restrict__ dqkv, int N, int H, float scale, float scale_log2e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NT = NKT + (NKT & 1);      // key tiles rounded to whole 32-key steps
  constexpr int NR = NT * 16;              // rows of every image
  constexpr int KS = (NKT + NW - 1) / NW;  // key tiles a wave may own
  constexpr int AB_THREADS = 64 * NW;      // NW = 4: one wave per SIMD; NW = 8: two (the same LDS images, half the tiles per wave)
  static_assert(NW == 4 || NW == 8, "4 or 8 waves");
  char* Qs = smem;
  char* Ks = Qs + NR * 128;
  char* Vs = Ks + NR * 128;
  char* Ds = Vs + NR * 128;                // dO
  char* Si = Ds + NR * 128;                // dS image [32 queries][DS_ROW bytes]
  float* L2 = reinterpret_cast<float*>(Si + DS_BYTES);
  float* Dl = L2 + NR;

  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
  const int64_t ts3 = (int64_t)3 * H * ATT_D, ts1 = (int64_t)H * ATT_D;   // elements between tokens: qkv / o, dout
  const HT* qbase = qkv + (int64_t)b * N * ts3 + h * ATT_D;
  const HT* obase = o + (int64_t)b * N * ts1 + h * ATT_D;
  const HT* dbase = dout + (int64_t)b * N * ts1 + h * ATT_D;
  HT* gbase = dqkv + (int64_t)b * N * ts3 + h * ATT_D;

  // ---- stage Q, K, V, dO (LDS DMA, 8 rows per wave-instruction, swizzle on the source address) ------------------------------
  for (int pc = wave; pc < NR / 8; pc += NW) {
    const HT* p3 = qbase + piece_off<false>(ts3, N, pc, lane);
    stage_piece(Qs, pc, p3);
    stage_piece(Ks, pc, p3 + H * ATT_D);
    stage_piece(Vs, pc, p3 + 2 * H * ATT_D);
    stage_piece(Ds, pc, dbase + piece_off<false>(ts1, N, pc, lane));
  }
  // the dS image starts out zero: the columns of the padding tile (keys NKT*16 .. NT*16) are never written
  for (int i = tid; i < DS_BYTES / 16; i += AB_THREADS) reinterpret_cast<u32x4*>(Si)[i] = u32x4{0u, 0u, 0u, 0u};
  // per-query constants: lse and delta = rowsum(dO O)
  for (int q = tid; q < NR; q += AB_THREADS) {
    const int sq = q < N ? q : N - 1;
    float dl = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c)
      dl = dot8<HT>(*reinterpret_cast<const u32x4*>(obase + (int64_t)sq * ts1 + c * 8),
                    *reinterpret_cast<const u32x4*>(dbase + (int64_t)sq * ts1 + c * 8), dl);
    Dl[q] = dl;
    L2[q] = lse[((int64_t)b * H + h) * N + sq];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  f32x4 dVa[KS][4], dKa[KS][4];
#pragma unroll
  for (int i = 0; i < KS; ++i)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dVa[i][dt] = dKa[i][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nsteps = (N + 31) >> 5;
  for (int qs = 0; qs < nsteps; ++qs) {
    const int q0 = qs * 32;
    // ---------------------------------------------------------------- phase A: own key tiles, all 32 queries of the step
    u32x4 qf[2][2], df[2][2], dOT[4], QT[4];
    f32x4 l2v[2], dlv[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        qf[t][kk] = *reinterpret_cast<const u32x4*>(Qs + img_off(q0 + 16 * t + li, 4 * kk + g));
        df[t][kk] = *reinterpret_cast<const u32x4*>(Ds + img_off(q0 + 16 * t + li, 4 * kk + g));
      }
      l2v[t] = *reinterpret_cast<const f32x4*>(L2 + q0 + 16 * t + 4 * g);
      dlv[t] = *reinterpret_cast<const f32x4*>(Dl + q0 + 16 * t + 4 * g);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dOT[dt] = tr_pair(Ds, q0 + 4 * g, q0 + 16 + 4 * g, dt, tq, tp);
      QT[dt] = tr_pair(Qs, q0 + 4 * g, q0 + 16 + 4 * g, dt, tq, tp);
    }
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const int kt = wave + NW * i;
      if (kt < NKT) {        // wave-uniform
        u32x4 kf[2], vf[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          kf[kk] = *reinterpret_cast<const u32x4*>(Ks + img_off(kt * 16 + li, 4 * kk + g));
          vf[kk] = *reinterpret_cast<const u32x4*>(Vs + img_off(kt * 16 + li, 4 * kk + g));
        }
        f32x4 S[2], dP[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          S[t] = mma<HT>(qf[t][0], kf[0], f32x4{0.f, 0.f, 0.f, 0.f});
          dP[t] = mma<HT>(df[t][0], vf[0], f32x4{0.f, 0.f, 0.f, 0.f});
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          S[t] = mma<HT>(qf[t][1], kf[1], S[t]);
          dP[t] = mma<HT>(df[t][1], vf[1], dP[t]);
        }
        const int key = kt * 16 + li;
        const bool kvalid = key < N;
        f32x4 P[2], dS[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool valid = kvalid && (q0 + 16 * t + 4 * g + r < N);
            const float p = valid ? __builtin_amdgcn_exp2f(fmaf(S[t][r], scale_log2e, -l2v[t][r])) : 0.f;
            P[t][r] = p;
            dS[t][r] = p * (dP[t][r] - dlv[t][r]) * scale;
          }
        const u32x4 pb = pack8<HT>(P[0], P[1]), sb = pack8<HT>(dS[0], dS[1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dVa[i][dt] = mma<HT>(dOT[dt], pb, dVa[i][dt]);
          dKa[i][dt] = mma<HT>(QT[dt], sb, dKa[i][dt]);
        }
        // dS -> LDS image [query row][key], 16-bit: phase B's contraction runs over the keys
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * t + 4 * g + r;
            const unsigned short v = (unsigned short)((r & 1) ? (sb[2 * t + (r >> 1)] >> 16) : (sb[2 * t + (r >> 1)] & 0xffffu));
            *reinterpret_cast<unsigned short*>(Si + row * DS_ROW + ((((key >> 3) ^ (row & 15))) << 4) + (key & 7) * 2) = v;
          }
      }
    }
    __syncthreads();
    // ---------------------------------------------------------------- phase B: dQ^T rows 16 w .. 16 w + 15, all keys
    // (NW = 8: wave w takes head-dim block w & 3 for the 16 queries of sub-tile w >> 2 only)
    {
      constexpr int TB = NW == 4 ? 2 : 1;                 // query sub-tiles per wave
      const int db = wave & 3, t0 = NW == 4 ? 0 : (wave >> 2);
      f32x4 dQ[TB];
#pragma unroll
      for (int t = 0; t < TB; ++t) dQ[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NT / 2; ++ks) {
        const u32x4 ka = tr_pair(Ks, 32 * ks + 8 * g, 32 * ks + 8 * g + 4, db, tq, tp);
#pragma unroll
        for (int t = 0; t < TB; ++t) {
          const int row = 16 * (t0 + t) + li;
          const u32x4 sv = *reinterpret_cast<const u32x4*>(Si + row * DS_ROW + (((4 * ks + g) ^ (row & 15)) << 4));
          dQ[t] = mma<HT>(ka, sv, dQ[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < TB; ++t) {
        const int q = q0 + 16 * (t0 + t) + li;
        if (q < N) *reinterpret_cast<u32x2*>(gbase + (int64_t)q * ts3 + 16 * db + 4 * g) = cvt4<HT>(dQ[t]);
      }
    }
    __syncthreads();   // the image is rewritten by the next step's phase A
  }
  // ---- dK, dV of the owned key tiles: lane (g, key li) holds head-dim elements 16 dt + 4 g + r -----------------------------
#pragma unroll
  for (int i = 0; i < KS; ++i) {
    const int kt = wave + NW * i;
    const int key = kt * 16 + li;
    if (kt < NKT && key < N) {
      HT* kp = gbase + (int64_t)key * ts3 + H * ATT_D + 4 * g;
      store_tile(kp, dKa[i]);
      store_tile(kp + H * ATT_D, dVa[i]);
    }
  }
}

template <typename HT, int NKT, int NW>
int launch_bwd(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, int B, int N, int H, float scale,
               hipStream_t s) {
  constexpr int NT = NKT + (NKT & 1);
  const size_t smem = 4 * (size_t)NT * 16 * 128 + DS_BYTES + 2 * (size_t)NT * 16 * sizeof(float);
  SMOE_ENSURE_SMEM((attn_bwd_kernel<HT, NKT, NW>));
  hipLaunchKernelGGL((attn_bwd_kernel<HT, NKT, NW>), dim3(B * H), dim3(64 * NW), smem, s, (const HT*)qkv, (const HT*)o,
                     (const HT*)dout, lse, (HT*)dqkv, N, H, scale, scale * 1.4426950408889634f);
  SMOE_CHECK_LAUNCH("smoe_attention_bwd");
  return 0;
}

// ---- long sequences (256 < N <= 640; ViT-L/16 @384: N = 577, models/vision_transformer.py:1227-1236) ---------------------------
// Q, K, V and dO of a head no longer fit the LDS together (4 x 577 x 128 B = 303 KB), so the work is split into two kernels that
// each finish their outputs alone -- no reduction across workgroups, waves or launches, no atomics, the same bits on every call:
//   attn_bwd_dkv_kernel  one workgroup (8 waves) per (image, head, block of 128 keys); wave w owns key tile 8 kb + w, its K / V row
//                        fragments stay in registers and Q / dO are streamed through LDS in 32-query steps (register-staged,
//                        double-buffered, one barrier per step).  A step is phase A of attn_bwd_kernel with KS = 1; there is no dS
//                        image and no phase B.
//   attn_bwd_dq_kernel   the long forward's skeleton without the softmax: one workgroup (8 waves) per (image, head), K and V whole
//                        in LDS, each wave walks query tiles wave, wave + 8, ... and the keys in chunks of ABL_CH tiles with the KEYS
//                        on the M side (S^T = K Q^T, dP^T = V dO^T), so the dS^T accumulators pack straight into the B operand of
//                        dQ^T += K^T dS^T (A = transposed reads of K).  dQ of a tile lives in 4 x f32x4 over the whole key walk.
// S and dP are computed in both (14 N^2 64 FLOP per (image, head) instead of 10): the price of needing no reduction.
// delta = rowsum(dO O) is recomputed where it is needed (per staged step / per query tile), as attn_bwd_kernel does.
constexpr int ABL_THREADS = 512;
constexpr int ABL_KB = 128;                               // keys per workgroup of the dK / dV kernel: one 16-key tile per wave
constexpr int ABL_STEP = 2 * 32 * 128 + 2 * 32 * 4;       // a staged step: Q and dO images of 32 queries, their lse and delta
constexpr int ABL_CH = 4;                                 // key tiles per chunk of the dQ kernel

template <typename HT>
__global__ __launch_bounds__(ABL_THREADS, 4) void attn_bwd_dkv_kernel(const HT* __restrict__ qkv, const HT* __restrict__ o,
                                                                      const HT* __restrict__ dout, const float* __restrict__ lse,
                                                                      HT* __restrict__ dqkv, int N, int H, int nkb, float scale,
                                                                      float scale_log2e) {
  __shared__ __attribute__((aligned(16))) char smem[2 * ABL_STEP];
  const int kb = blockIdx.x % nkb, bh = blockIdx.x / nkb, b = bh / H, h = bh % H;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
  const int64_t ts3 = (int64_t)3 * H * ATT_D, ts1 = (int64_t)H * ATT_D;
  const HT* qbase = qkv + (int64_t)b * N * ts3 + h * ATT_D;
  const HT* obase = o + (int64_t)b * N * ts1 + h * ATT_D;
  const HT* dbase = dout + (int64_t)b * N * ts1 + h * ATT_D;
  const float* lbase = lse + ((int64_t)b * H + h) * N;
  HT* gbase = dqkv + (int64_t)b * N * ts3 + h * ATT_D;

  // the wave's key tile: K / V row fragments straight from memory (keys >= N duplicate row N - 1 and carry P = dS = 0)
  const int kt = kb * (ABL_KB / 16) + wave;
  const int key = kt * 16 + li;
  const bool kvalid = key < N;
  const bool tile_live = kt * 16 < N;      // wave-uniform
  u32x4 kf[2], vf[2];
  {
    const HT* kp = qbase + (int64_t)(kvalid ? key : N - 1) * ts3 + H * ATT_D + g * 8;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      kf[kk] = *reinterpret_cast<const u32x4*>(kp + 32 * kk);
      vf[kk] = *reinterpret_cast<const u32x4*>(kp + H * ATT_D + 32 * kk);
    }
  }
  // staging roles: waves 0-3 carry the Q image of a step (one 16-byte piece per thread), waves 4-7 the dO image, the O piece next
  // to it (delta) and the row's lse
  const bool is_q = wave < 4;              // wave-uniform
  const int s_row = (tid & 255) >> 3, s_c = tid & 7;
  u32x4 piece = u32x4{0u, 0u, 0u, 0u}, opiece = piece;
  float lv = 0.f;
  auto fetch = [&](int qs) {
    const int row = qs * 32 + s_row;
    const int srow = row < N ? row : N - 1;
    if (is_q) {
      piece = *reinterpret_cast<const u32x4*>(qbase + (int64_t)srow * ts3 + s_c * 8);
    } else {
      piece = *reinterpret_cast<const u32x4*>(dbase + (int64_t)srow * ts1 + s_c * 8);
      opiece = *reinterpret_cast<const u32x4*>(obase + (int64_t)srow * ts1 + s_c * 8);
      lv = lbase[srow];
    }
  };
  auto commit = [&](int buf) {
    char* st = smem + buf * ABL_STEP;
    if (is_q) {
      *reinterpret_cast<u32x4*>(st + img_off(s_row, s_c)) = piece;
    } else {
      *reinterpret_cast<u32x4*>(st + 32 * 128 + img_off(s_row, s_c)) = piece;
      float dl = dot8<HT>(opiece, piece);
      dl += __shfl_xor(dl, 1, 64);
      dl += __shfl_xor(dl, 2, 64);
      dl += __shfl_xor(dl, 4, 64);
      if (s_c == 0) {
        float* f = reinterpret_cast<float*>(st + 2 * 32 * 128);
        f[s_row] = lv;
        f[32 + s_row] = dl;
      }
    }
  };

  f32x4 dVa[4], dKa[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dVa[dt] = dKa[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nsteps = (N + 31) >> 5;
  fetch(0);
  commit(0);
  __syncthreads();
  for (int qs = 0; qs < nsteps; ++qs) {
    if (qs + 1 < nsteps) fetch(qs + 1);          // the next step's loads fly under this step's math
    if (tile_live) {
      const char* Qs = smem + (qs & 1) * ABL_STEP;
      const char* Ds = Qs + 32 * 128;
      const float* L2 = reinterpret_cast<const float*>(Qs + 2 * 32 * 128);
      const float* Dl = L2 + 32;
      const int q0 = qs * 32;
      u32x4 qf[2][2], df[2][2];
      f32x4 l2v[2], dlv[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          qf[t][kk] = *reinterpret_cast<const u32x4*>(Qs + img_off(16 * t + li, 4 * kk + g));
          df[t][kk] = *reinterpret_cast<const u32x4*>(Ds + img_off(16 * t + li, 4 * kk + g));
        }
      }
      f32x4 S[2], dP[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        S[t] = mma<HT>(qf[t][0], kf[0], f32x4{0.f, 0.f, 0.f, 0.f});
        dP[t] = mma<HT>(df[t][0], vf[0], f32x4{0.f, 0.f, 0.f, 0.f});
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        S[t] = mma<HT>(qf[t][1], kf[1], S[t]);
        dP[t] = mma<HT>(df[t][1], vf[1], dP[t]);
      }
      __builtin_amdgcn_sched_barrier(0);       // (register budget: lse / delta are read once the Q / dO fragments are dead)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        l2v[t] = *reinterpret_cast<const f32x4*>(L2 + 16 * t + 4 * g);
        dlv[t] = *reinterpret_cast<const f32x4*>(Dl + 16 * t + 4 * g);
      }
      f32x4 P[2], dS[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool valid = kvalid && (q0 + 16 * t + 4 * g + r < N);
          const float p = __builtin_amdgcn_exp2f(fmaf(S[t][r], scale_log2e, -l2v[t][r]));
          P[t][r] = valid ? p : 0.f;                                       // selected away, never multiplied away
          dS[t][r] = valid ? p * (dP[t][r] - dlv[t][r]) * scale : 0.f;
        }
      const u32x4 pb = pack8<HT>(P[0], P[1]), sb = pack8<HT>(dS[0], dS[1]);
      // the transposed A operands are read only now: with S / dP still live they would not fit 128 registers (4 waves per SIMD)
      __builtin_amdgcn_sched_barrier(0);
      u32x4 at[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) at[dt] = tr_pair(Ds, 4 * g, 16 + 4 * g, dt, tq, tp);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) dVa[dt] = mma<HT>(at[dt], pb, dVa[dt]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) at[dt] = tr_pair(Qs, 4 * g, 16 + 4 * g, dt, tq, tp);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) dKa[dt] = mma<HT>(at[dt], sb, dKa[dt]);
    }
    if (qs + 1 < nsteps) commit((qs + 1) & 1);   // that buffer was last read in step qs - 1, a barrier ago
    __syncthreads();
  }
  if (kvalid) {
    HT* kp = gbase + (int64_t)key * ts3 + H * ATT_D + 4 * g;
    store_tile(kp, dKa);
    store_tile(kp + H * ATT_D, dVa);
  }
}

// nkt_pad = key tiles held in LDS: ceil(N / 16) rounded up to whole chunks (rows >= N duplicate row N - 1)
template <typename HT>
__global__ __launch_bounds__(ABL_THREADS, 1) void attn_bwd_dq_kernel(const HT* __restrict__ qkv, const HT* __restrict__ o,
                                                                        const HT* __restrict__ dout, const float* __restrict__ lse,
                                                                        HT* __restrict__ dqkv, int N, int H, int nkt_pad, float scale,
                                                                        float scale_log2e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + nkt_pad * 16 * 128;
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
  const int64_t ts3 = (int64_t)3 * H * ATT_D, ts1 = (int64_t)H * ATT_D;
  const HT* qbase = qkv + (int64_t)b * N * ts3 + h * ATT_D;
  const HT* obase = o + (int64_t)b * N * ts1 + h * ATT_D;
  const HT* dbase = dout + (int64_t)b * N * ts1 + h * ATT_D;
  const float* lbase = lse + ((int64_t)b * H + h) * N;
  HT* gbase = dqkv + (int64_t)b * N * ts3 + h * ATT_D;
  // ---- stage K and V of the head (LDS DMA, 8 rows per wave-instruction, swizzle on the source address; both images in the
  //      row-read layout of img_off: K is read by rows AND transposed, V by rows only) ------------------------------------------------
  for (int pc = wave; pc < nkt_pad * 2; pc += ABL_THREADS / 64) {
    const HT* p3 = qbase + H * ATT_D + piece_off<false>(ts3, N, pc, lane);
    stage_piece(Ks, pc, p3);
    stage_piece(Vs, pc, p3 + H * ATT_D);
  }
  const int nqt = (N + 15) >> 4;
  const int nchunk = nkt_pad / ABL_CH;
  // a query tile's operands: Q / dO row fragments (the B operands of S^T / dP^T, held over the whole key walk), lse and delta of
  // the lane's query (the 4 lanes that share a query each sum a quarter of dO O)
  struct Tile { u32x4 q0, q1, d0, d1; float l2, dl; };
  auto load_tile = [&](int qt, Tile& t) {
    u32x4 o0, o1;
    load_q(qbase, ts3, N, qt, li, g, t.q0, t.q1);
    load_q(dbase, ts1, N, qt, li, g, t.d0, t.d1);
    load_q(obase, ts1, N, qt, li, g, o0, o1);
    t.l2 = lbase[min(qt * 16 + li, N - 1)];
    float dl = dot8<HT>(o0, t.d0) + dot8<HT>(o1, t.d1);
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    t.dl = dl;
  };
  Tile nxt = {};
  if (wave < nqt) load_tile(wave, nxt);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int qt = wave; qt < nqt; qt += ABL_THREADS / 64) {
    const Tile cur = nxt;
    if (qt + ABL_THREADS / 64 < nqt) load_tile(qt + ABL_THREADS / 64, nxt);   // next tile's operands under this tile's math
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
      const int t0 = __builtin_amdgcn_readfirstlane(c * ABL_CH);
      f32x4 S[ABL_CH], dP[ABL_CH];
      u32x4 kf[ABL_CH][2], vf[ABL_CH][2];
#pragma unroll
      for (int i = 0; i < ABL_CH; ++i)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          kf[i][kk] = *reinterpret_cast<const u32x4*>(Ks + img_off((t0 + i) * 16 + li, 4 * kk + g));
          vf[i][kk] = *reinterpret_cast<const u32x4*>(Vs + img_off((t0 + i) * 16 + li, 4 * kk + g));
        }
#pragma unroll
      for (int i = 0; i < ABL_CH; ++i) {
        S[i] = mma<HT>(kf[i][0], cur.q0, f32x4{0.f, 0.f, 0.f, 0.f});
        dP[i] = mma<HT>(vf[i][0], cur.d0, f32x4{0.f, 0.f, 0.f, 0.f});
      }
#pragma unroll
      for (int i = 0; i < ABL_CH; ++i) {
        S[i] = mma<HT>(kf[i][1], cur.q1, S[i]);
        dP[i] = mma<HT>(vf[i][1], cur.d1, dP[i]);
      }
      // lane (g, query li) holds keys 16 (t0 + i) + 4 g + r; keys >= N are selected away
#pragma unroll
      for (int i = 0; i < ABL_CH; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool valid = (t0 + i) * 16 + 4 * g + r < N;
          const float p = __builtin_amdgcn_exp2f(fmaf(S[i][r], scale_log2e, -cur.l2));
          S[i][r] = valid ? p * (dP[i][r] - cur.dl) * scale : 0.f;
        }
      // dQ^T += K^T dS^T over the chunk's k-steps of 32 keys: k-slot (g, j) <-> key 16 (t0 + 2 ks + (j >> 2)) + 4 g + (j & 3)
#pragma unroll
      for (int ks = 0; ks < ABL_CH / 2; ++ks) {
        const u32x4 sb = pack8<HT>(S[2 * ks], S[2 * ks + 1]);
        const int ra = (t0 + 2 * ks) * 16 + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[dt] = mma<HT>(tr_pair(Ks, ra, ra + 16, dt, tq, tp), sb, dq[dt]);
      }
    }
    // ---- store: lane (g, li) holds head-dim elements 16 dt + 4 g + r of query 16 qt + li ------------------------------------------
    const int q = qt * 16 + li;
    if (q < N) store_tile(gbase + (int64_t)q * ts3 + 4 * g, dq);
  }
}

template <typename HT>
int launch_bwd_long(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, int B, int N, int H, float scale,
                    hipStream_t s) {
  const int nkt = (N + 15) / 16;
  const int nkt_pad = (nkt + ABL_CH - 1) / ABL_CH * ABL_CH;       // <= 40 tiles: 160 KB, what the long forward asks for
  const size_t smem = 2 * (size_t)nkt_pad * 16 * 128;
  const int nkb = (N + ABL_KB - 1) / ABL_KB;
  const float sl2 = scale * 1.4426950408889634f;
  SMOE_ENSURE_SMEM(attn_bwd_dq_kernel<HT>);
  hipLaunchKernelGGL((attn_bwd_dq_kernel<HT>), dim3(B * H), dim3(ABL_THREADS), smem, s, (const HT*)qkv, (const HT*)o, (const HT*)dout,
                     lse, (HT*)dqkv, N, H, nkt_pad, scale, sl2);
  SMOE_CHECK_LAUNCH("smoe_attention_bwd/dq");
  hipLaunchKernelGGL((attn_bwd_dkv_kernel<HT>), dim3(B * H * nkb), dim3(ABL_THREADS), 0, s, (const HT*)qkv, (const HT*)o,
                     (const HT*)dout, lse, (HT*)dqkv, N, H, nkb, scale, sl2);
  SMOE_CHECK_LAUNCH("smoe_attention_bwd/dkv");
  return 0;
}

// waves per workgroup: the images fill the LDS (one workgroup per CU), so 8 waves = two per SIMD is what hides the latencies between
// a step's dependent phases (LDS reads -> MFMA -> exp / pack -> MFMA); SMOE_ATTN_BWD_WAVES=4 keeps one per SIMD (A/B)
inline int bwd_waves() {
  static const int w = [] { const char* e = getenv("SMOE_ATTN_BWD_WAVES"); return (e && atoi(e) == 4) ? 4 : 8; }();
  return w;
}

template <typename HT>
int bwd_dispatch(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, int B, int N, int H, float scale,
                 hipStream_t s) {
  const int nkt = (N + 15) / 16;
  if (nkt > 16) return launch_bwd_long<HT>(qkv, o, dout, lse, dqkv, B, N, H, scale, s);   // SMOE_ATTN_BWD_WAVES does not reach these
  if (nkt <= 4) return launch_bwd<HT, 4, 4>(qkv, o, dout, lse, dqkv, B, N, H, scale, s);
  if (nkt <= 8) return bwd_waves() == 8 ? launch_bwd<HT, 8, 8>(qkv, o, dout, lse, dqkv, B, N, H, scale, s)
                                        : launch_bwd<HT, 8, 4>(qkv, o, dout, lse, dqkv, B, N, H, scale, s);
  if (nkt <= 13) return bwd_waves() == 8 ? launch_bwd<HT, 13, 8>(qkv, o, dout, lse, dqkv, B, N, H, scale, s)   // N = 197 / 198
                                         : launch_bwd<HT, 13, 4>(qkv, o, dout, lse, dqkv, B, N, H, scale, s);
  return bwd_waves() == 8 ? launch_bwd<HT, 16, 8>(qkv, o, dout, lse, dqkv, B, N, H, scale, s)
                          : launch_bwd<HT, 16, 4>(qkv, o, dout, lse, dqkv, B, N, H, scale, s);
}

}  // namespace

extern "C" int smoe_attention_bwd_supported(int N, int head_dim) { return (N >= 1 && N <= 640 && head_dim == ATT_D) ? 1 : 0; }

// qkv, dqkv [B, N, 3, H, 64]; o, dout [B, N, H*64]; lse [B, H, N] f32 from smoe_attention_fwd; f16 or bf16
extern "C" int smoe_attention_bwd(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, int dtype, int B,
                                  int N, int H, int head_dim, float scale, void* stream) {
  SMOE_REQUIRE(smoe_attention_bwd_supported(N, head_dim), "smoe_attention_bwd: unsupported N=%d head_dim=%d (N <= 640, head dim 64)",
               N, head_dim);
  SMOE_REQUIRE(B >= 0 && H >= 1, "smoe_attention_bwd: bad B=%d H=%d", B, H);
  if (B == 0) return 0;
  SMOE_REQUIRE(qkv && o && dout && lse && dqkv, "smoe_attention_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SMOE_F16) return bwd_dispatch<f16>(qkv, o, dout, lse, dqkv, B, N, H, scale, s);
  if (dtype == SMOE_BF16) return bwd_dispatch<bf16_bits>(qkv, o, dout, lse, dqkv, B, N, H, scale, s);
  smoe_set_error("smoe_attention_bwd: dtype must be f16 or bf16");
  return 1;
}
