// Counter-based dropout (main.py --drop: models/vision_transformer.py pos_drop / proj_drop, models/resMoE.py's expert Dropout behind
// GELU).  The mask is never stored: it is a pure function of (key, first_block, element index), so the backward regenerates it
// (dx = dropout_with_the_same_key(dy)) and the host can reproduce it bit for bit (tests/_dropout_cases.py).
//   smoe_dropout      : y = rn(select(kept, f32(x) * scale [* row_scale[row]], +0))      -- every forward that adds nothing, every backward
//   smoe_dropout_add  : out_f32 = residual_f32 + select(kept, f32(h) * scale [* row_scale[row]], +0)   -- x + drop_path(proj_drop(proj(o)))
// THE RULE.  Philox4x32-10 (Random123 constants).  The key is a DEVICE tensor int64[2] = (k, c), read from memory on every launch (a
// captured launch sees the key its replay drew).  Elements are numbered row-major over [rows, cols], cols % 8 == 0; element e lies in
// block b = first_block + e / 8; the Philox key of block b is (lo32 k, hi32 k), its counter (lo32 b, hi32 b, lo32 c, hi32 c); of the
// four output words r0..r3, element 8 b + 2 j + h draws u = (r_j >> 16 h) & 0xffff and is kept iff u < thr16 (thr16 = round(keep *
// 65536), 0 .. 65536).  scale = (float)(65536.0 / thr16), 0 for thr16 == 0: the inverse of the keep probability really applied.  All
// arithmetic in f32, one rounding per operation (no contraction), one rounding into the output dtype.  A dropped element is SELECTED to
// +0.0, never multiplied by 0: a dropped NaN / inf gives 0, a kept one propagates.
// One Philox call per lane and trip = 8 elements = one 16-byte access of 16-bit data (two of f32); 256 threads; the grid is capped at
// DROP_MAX_BLOCKS workgroups with a grid stride behind it; 64-bit indices; plain vector stores, no LDS, no atomics.
#include "smoe_common.h"

namespace {

constexpr int DROP_THREADS = 256;
constexpr int DROP_MAX_BLOCKS = 4096;   // smoe_cast's cap: 16 workgroups per CU

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&r)[4]) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += W0;
    k1 += W1;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// one rounding per operation: the empty asm keeps the product out of a following FMA / mixed-precision convert
__device__ __forceinline__ float mul_rn(float a, float b) {
  float t = __fmul_rn(a, b);
  asm volatile("" : "+v"(t));
  return t;
}
__device__ __forceinline__ float add_rn(float a, float b) {
  float t = __fadd_rn(a, b);
  asm volatile("" : "+v"(t));
  return t;
}

// x, y (and residual) are NOT __restrict__: y may be x, out may be residual -- every lane reads its 8 elements before it writes them
template <typename TI, typename TO, bool ADD>
__global__ __launch_bounds__(DROP_THREADS) void dropout_kernel(const TI* x, TO* y, const float* residual,
                                                               const float* __restrict__ row_scale,
                                                               const uint64_t* __restrict__ key, uint64_t first_block,
                                                               int64_t n_blocks, int64_t cols8, uint32_t thr16, float scale) {
  const uint64_t k = key[0], c = key[1];
  const uint32_t k0 = (uint32_t)k, k1 = (uint32_t)(k >> 32), c2 = (uint32_t)c, c3 = (uint32_t)(c >> 32);
  const bool narrow = n_blocks <= 0xffffffffll;   // the row of a block by a 32-bit division where that is exact
  const int64_t stride = (int64_t)gridDim.x * DROP_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * DROP_THREADS + threadIdx.x; i < n_blocks; i += stride) {
    const uint64_t b = first_block + (uint64_t)i;
    uint32_t r[4];
    philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), c2, c3, k0, k1, r);
    float v[8], res[8];
    load8(x + i * 8, v);
    if constexpr (ADD) load8(residual + i * 8, res);
    float rs = 1.0f;
    if (row_scale) rs = row_scale[narrow ? (int64_t)((uint32_t)i / (uint32_t)cols8) : i / cols8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint32_t u = (r[q >> 1] >> (16 * (q & 1))) & 0xffffu;
      float t = mul_rn(v[q], scale);
      if (row_scale) t = mul_rn(t, rs);
      t = u < thr16 ? t : 0.0f;
      if constexpr (ADD) t = add_rn(res[q], t);
      v[q] = t;
    }
    store8(y + i * 8, v);
  }
}

template <typename TI, typename TO, bool ADD>
int launch(const void* x, void* y, const float* residual, const float* row_scale, const int64_t* key, uint64_t first_block,
           int64_t rows, int64_t cols, uint32_t thr16, float scale, hipStream_t s, const char* name) {
  const int64_t n_blocks = rows * (cols / 8);
  int64_t grid = (n_blocks + DROP_THREADS - 1) / DROP_THREADS;
  if (grid > DROP_MAX_BLOCKS) grid = DROP_MAX_BLOCKS;
  hipLaunchKernelGGL((dropout_kernel<TI, TO, ADD>), dim3((unsigned)grid), dim3(DROP_THREADS), 0, s, (const TI*)x, (TO*)y, residual,
                     row_scale, reinterpret_cast<const uint64_t*>(key), first_block, n_blocks, cols / 8, thr16, scale);
  SMOE_CHECK_LAUNCH(name);
  return 0;
}

template <typename TI, bool ADD>
int launch_out(int dtype_out, const void* x, void* y, const float* residual, const float* row_scale, const int64_t* key,
               uint64_t first_block, int64_t rows, int64_t cols, uint32_t thr16, float scale, hipStream_t s, const char* name) {
  switch (dtype_out) {
    case SMOE_F32: return launch<TI, float, ADD>(x, y, residual, row_scale, key, first_block, rows, cols, thr16, scale, s, name);
    case SMOE_F16: return launch<TI, f16, ADD>(x, y, residual, row_scale, key, first_block, rows, cols, thr16, scale, s, name);
    default: return launch<TI, bf16_bits, ADD>(x, y, residual, row_scale, key, first_block, rows, cols, thr16, scale, s, name);
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the size checks both entry points share; rows * cols elements of up to 4 bytes are addressed in int64
#define DROP_CHECK_SIZES(name)                                                                                                   \
  SMOE_REQUIRE(rows >= 0 && cols > 0 && cols % 8 == 0, name ": rows=%lld, cols=%lld: cols must be a positive multiple of 8",      \
               (long long)rows, (long long)cols);                                                                                \
  SMOE_REQUIRE(thr16 <= 65536u, name ": thr16=%u is outside [0, 65536]", thr16);                                                  \
  SMOE_REQUIRE(rows <= (INT64_MAX / 4) / cols, name ": rows * cols overflows the 64-bit byte index (rows=%lld, cols=%lld)",       \
               (long long)rows, (long long)cols)

}  // namespace

extern "C" int smoe_dropout(const void* x, void* y, const float* row_scale, const int64_t* key, uint64_t first_block, int64_t rows,
                            int64_t cols, uint32_t thr16, float scale, int dtype_in, int dtype_out, void* stream) {
  SMOE_REQUIRE(smoe_dtype_ok(dtype_in) && smoe_dtype_ok(dtype_out), "smoe_dropout: unknown dtype (in %d, out %d)", dtype_in, dtype_out);
  DROP_CHECK_SIZES("smoe_dropout");
  SMOE_REQUIRE(x && y && key, "smoe_dropout: null pointer");
  SMOE_REQUIRE(aligned(x, 16) && aligned(y, 16), "smoe_dropout: x and y must be 16-byte aligned");
  SMOE_REQUIRE(aligned(key, 8) && aligned(row_scale, 4), "smoe_dropout: misaligned key (8 bytes) or row_scale (4 bytes)");
  SMOE_REQUIRE(x != y || dtype_in == dtype_out, "smoe_dropout: y may be x only when the dtypes are equal");
  if (rows == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  switch (dtype_in) {
    case SMOE_F32: return launch_out<float, false>(dtype_out, x, y, nullptr, row_scale, key, first_block, rows, cols, thr16, scale, s, "smoe_dropout");
    case SMOE_F16: return launch_out<f16, false>(dtype_out, x, y, nullptr, row_scale, key, first_block, rows, cols, thr16, scale, s, "smoe_dropout");
    default: return launch_out<bf16_bits, false>(dtype_out, x, y, nullptr, row_scale, key, first_block, rows, cols, thr16, scale, s, "smoe_dropout");
  }
}

extern "C" int smoe_dropout_add(const void* h, const float* residual, const float* row_scale, float* out, const int64_t* key,
                                uint64_t first_block, int64_t rows, int64_t cols, uint32_t thr16, float scale, int dtype_h,
                                void* stream) {
  SMOE_REQUIRE(smoe_dtype_ok(dtype_h), "smoe_dropout_add: unknown dtype %d", dtype_h);
  DROP_CHECK_SIZES("smoe_dropout_add");
  SMOE_REQUIRE(h && residual && out && key, "smoe_dropout_add: null pointer");
  SMOE_REQUIRE(aligned(h, 16) && aligned(residual, 16) && aligned(out, 16), "smoe_dropout_add: h, residual and out must be 16-byte aligned");
  SMOE_REQUIRE(aligned(key, 8) && aligned(row_scale, 4), "smoe_dropout_add: misaligned key (8 bytes) or row_scale (4 bytes)");
  SMOE_REQUIRE((const void*)out != h, "smoe_dropout_add: out may be the residual, never h");
  if (rows == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  switch (dtype_h) {
    case SMOE_F32: return launch<float, float, true>(h, out, residual, row_scale, key, first_block, rows, cols, thr16, scale, s, "smoe_dropout_add");
    case SMOE_F16: return launch<f16, float, true>(h, out, residual, row_scale, key, first_block, rows, cols, thr16, scale, s, "smoe_dropout_add");
    default: return launch<bf16_bits, float, true>(h, out, residual, row_scale, key, first_block, rows, cols, thr16, scale, s, "smoe_dropout_add");
  }
}
