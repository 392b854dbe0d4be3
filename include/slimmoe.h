/* slimmoe.h -- C-ABI of libslimmoe_hip.so: MI355X (gfx950) kernels for the Switch-MoE ViT hot path.
 *
 * Drop-in boundary.  The reference (d0-rb/slim-switch-moe-vit) has no FFI of its own: its MoE
 * operator is `from fmoe import FMoETransformerMLP` (models/resMoE.py:6, ctor at 27-29, forward at
 * 121/143 and models/vision_transformer.py:321), and FastMoE in turn binds a pybind module
 * `fmoe_cuda` (expert_count, assign_pos, linear_forward, limit_by_capacity, prune_gate_by_capacity,
 * global_scatter/gather ...).  The entry points below are what a binding
 * for that op set would bind; each comment names the upstream op it replaces.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *    (torch tensors), contiguous, 16-byte aligned; nothing here allocates, frees or synchronises;
 *  - process-global state is limited to (i) the thread-local error string and (ii) one atomic bit per
 *    (kernel, device) recording that the kernel's dynamic-LDS limit has been raised on that device, plus the
 *    cached CU count per device.  smoe_init() sets all of (ii) for the CURRENT device; call it once per device
 *    before capturing launches into a hipGraph (after it no entry point touches function attributes).  Without
 *    it the first launch of a kernel on a device sets its attribute itself (thread-safe: the update is an
 *    atomic OR and setting the attribute twice is harmless);
 *  - entry points may be called concurrently from several host threads and on several streams; buffers handed
 *    to concurrent calls (workspaces, outputs) must be distinct;
 *  - all launches go to `stream` (a hipStream_t passed as void*);
 *  - return 0 on success, non-zero on error; smoe_last_error() gives the thread-local message;
 *  - dtype codes: SMOE_F32 / SMOE_F16 / SMOE_BF16.
 */
#ifndef SLIMMOE_H
#define SLIMMOE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SMOE_F32 = 0, SMOE_F16 = 1, SMOE_BF16 = 2 };
enum { SMOE_GATE_NAIVE = 0, SMOE_GATE_SWITCH = 1 };
enum { SMOE_EPI_NONE = 0, SMOE_EPI_GELU = 1, SMOE_EPI_GELU_GRAD = 2 };

/* smoe_set_reserved_cus(n): the persistent grouped GEMM (variants 9-14: one workgroup per CU for the whole launch, with all of the
 * CU's LDS and registers) leaves n CUs free from now on (process-wide; 0 <= n <= 128; default 0).  A kernel on ANOTHER stream cannot
 * share a CU with it, so RCCL's all-to-all under the expert-parallel micro-batch pipeline ("overlapped with the
 * local GEMM on a second HIP stream") only overlaps the GEMMs if some CUs are left to it; results do not depend on n. */
int smoe_set_reserved_cus(int n);

/* library ABI version (bumped on any signature change) */
int smoe_abi_version(void);
/* first 16 hex digits of the sha256 over the sources this binary was built from (csrc/Makefile HASHED): lets the loader
 * refuse, and build() replace, a shipped binary that does not belong to the shipped sources */
const char* smoe_build_id(void);
/* raise the dynamic-LDS limit of every kernel of the library on the current device (see Conventions); idempotent */
int smoe_init(void);
/* message for the last non-zero return on this thread */
const char* smoe_last_error(void);

/* ---- router ------------------------------------------------------------------------------------
 * Replaces fmoe NaiveGate.forward / SwitchGate.forward (gate = nn.Linear(d,E): evidenced by
 * models/resmoe_flop_hook.py:7-8; selected at models/resMoE.py:26-29).
 *   logits = x @ wg^T + bg           routing decided as if accumulated in f64 and rounded once to f32:
 *                                    f32 fast path with a rigorous error bound, f64 re-do of a token when a
 *                                    deciding gap is inside the bound (gate_kind | SMOE_ROUTER_ALL_F64 forces f64 for all)
 *   NAIVE : (val, idx) = top-k(logits) [ties: lowest expert id; descending logit]; score = softmax(val)
 *   SWITCH: k == 1; p = softmax(logits + noise) over all E; idx = argmax; score = p[idx];
 *           probs (may be NULL) receives p [T,E] for the aux loss.
 * x [T,d] (x_dtype), wg [E,d] f32, bg [E] f32 or NULL, noise [T,E] f32 or NULL.
 * idx [T,k] i64, score [T,k] f32, logits_out [T,E] f32 or NULL.
 * Requires d % 8 == 0, d <= 2048, 1 <= k <= E, k <= 4.  workspace: smoe_router_workspace_bytes(T) bytes
 * (redo counter + list of tokens handed to the f64 pass).  The calls clear the counter words with a small launch of
 * their own -- unless the caller keeps ONE workspace per stream and says so (gate_kind | SMOE_ROUTER_WS_KEPT_ZERO;
 * smoe_gate_ln_router: with_ln | 2): every redo pass leaves the counter words zero on its way out, so a workspace that was
 * zero before its first use stays ready, and the clearing launch in front of every router call disappears.  (An all-f64 call
 * with LayerNorm runs its f32 pass without a redo pass behind it: it is not to be combined with a kept workspace.)      */
#define SMOE_ROUTER_ALL_F64 0x100      /* gate_kind flag of smoe_router_topk / smoe_ln_router_topk: every token through the f64 pass */
#define SMOE_ROUTER_WS_KEPT_ZERO 0x200 /* gate_kind flag of the same two: the workspace's counter words are zero on entry */
size_t smoe_router_workspace_bytes(int64_t T);
int smoe_router_topk(const void* x, int x_dtype, const float* wg, const float* bg, const float* noise,
                     int64_t T, int d, int E, int k, int gate_kind,
                     int64_t* idx, float* score, float* logits_out, float* probs,
                     void* workspace, size_t workspace_bytes, void* stream);

/* LayerNorm + router fused (block glue, models/vision_transformer.py:321 `mlp(norm2(x))`): xn = LN(x)*gamma+beta
 * is written as a 16-bit image (xn16: f16/bf16, may be NULL) and / or f32 (xn32, may be NULL) and routed exactly
 * as smoe_router_topk routes xn.  Shapes covered: smoe_ln_router_supported(d, E, k) (k <= 4; E <= 8 with
 * d in {192, 384, 768, 1024}, E <= 32 with d in {768, 1024}); workspace as smoe_router_workspace_bytes(T).
 * chunk_hist (may be NULL; i32 [ceil(T / tok)][E], tok = smoe_router_chunk_hist_tokens(d, E, k) > 0): the per-chunk expert
 * histogram of the routing (count_by_gate folded into the router pass: the f32 pass walks contiguous chunks of `tok` tokens and
 * counts what it decides, the redo pass adds the tokens it decides) -- smoe_dispatch_plan_hist then builds the plan without its
 * own counting launch.  Shapes whose router writes none report tok = 0 and ignore the pointer.                             */
int smoe_ln_router_supported(int d, int E, int k);
int smoe_router_chunk_hist_tokens(int d, int E, int k);
int smoe_ln_router_topk(const void* x, int x_dtype, const float* ln_gamma, const float* ln_beta, float ln_eps,
                        void* xn16, int xn16_dtype, float* xn32, const float* wg, const float* bg, const float* noise,
                        int64_t T, int d, int E, int k, int gate_kind, int64_t* idx, float* score,
                        float* logits_out, float* probs, int32_t* chunk_hist, void* workspace, size_t workspace_bytes,
                        void* stream);

/* Token-skip gate of the residual-MoE block (models/resMoE.py:32-85 `Gate`; used at 126-145), fused with the LayerNorm
 * in front of it and -- for the MoE half -- with the router behind it: ONE pass over the activations replaces
 * `x = norm(x); mask = gate(x); skip_tk = x * mask[..,0]; tk = x * mask[..,1]` (+ the router's own pass over tk).
 *   xn   = with_ln ? LN(x) * gamma + beta : x                                  x [T,d] f32
 *   z    = <xn, gate_w> + gate_b;   skipped <=> sigmoid(z) > *threshold  <=>  z > logit(*threshold)
 *          (decided as if z were accumulated in f64: f32 pass with an error bound + f64 redo, like the router;
 *           threshold is read from DEVICE memory -- the module's buffer -- so no host sync; NULL = gate disabled)
 *   xn16 [T,d] (f16/bf16, may be NULL): the operand image of `tk`: xn, zeros for skipped tokens
 *   xn32 [T,d] (f32, may be NULL): the residual image `tk + skip_tk` = xn, plus zero_out[d] (may be NULL) on skipped
 *          rows -- the MoE output every all-zero row receives (smoe_zero_row_output), so the caller never dispatches them
 *   mask [T,2] f32 (skip, keep) (may be NULL);  *skip_count += skipped tokens (may be NULL)
 *   E > 0: NaiveGate routing of `tk` (a skipped token routes as the zero row it is: by the gate bias):
 *          idx / score as smoe_router_topk; idx_plan [T,k] = idx, or -1 for skipped tokens (feed THIS to
 *          smoe_dispatch_plan).  E == 0: gate only (the attention half).
 * Shapes: smoe_gate_ln_router_supported(d, E, k): d in {192, 384, 768, 1024}, E <= 8, k <= 4.
 * workspace as smoe_router_workspace_bytes(T).                                                              */
int smoe_gate_ln_router_supported(int d, int E, int k);
int smoe_gate_ln_router(const void* x, int x_dtype, int with_ln, const float* ln_gamma, const float* ln_beta, float ln_eps,
                        const float* gate_w, const float* gate_b, const float* threshold, void* xn16, int xn16_dtype,
                        float* xn32, const float* zero_out, const float* wg, const float* bg, int64_t T, int d, int E,
                        int k, int64_t* idx, int64_t* idx_plan, float* score, float* mask, int32_t* skip_count,
                        int32_t* chunk_hist /* as smoe_ln_router_topk's; counts idx_plan's dispatched entries; may be NULL */,
                        float* tk32 /* [T,d] f32 or NULL: the (normed) row, ZEROS for a skipped token -- `x * mask[..., 1:]` of
                                       models/resMoE.py:141, the masked f32 image the training path's router and scatter read */,
                        void* workspace, size_t workspace_bytes, void* stream);
/* What the MoE returns for an all-zero input row (every token the skip gate masks, resMoE.py:140-143):
 *   out[d] = sum_j score_j (W2[e_j] gelu(b1[e_j]) + b2[e_j]),  (e_j, score_j) = NaiveGate top-k of the gate bias bg.
 * w2 [E,d,h], b1 [E,h], b2 [E,d], bg [E] f32 (b1 / b2 / bg may be NULL = zeros).  Depends on parameters only.  */
/* Under expert parallelism bg covers all E global experts while w2 / b1 / b2 hold the E_local experts [e_base, e_base + E_local)
 * of this rank: out is then this rank's PARTIAL sum (chosen experts that live elsewhere contribute nothing); the ranks' partial
 * sums add up to the full row (one all-reduce per parameter version).  Single rank: e_base = 0, E_local = E.                  */
int smoe_zero_row_output(const float* bg, int E, int k, const float* w2, const float* b1, const float* b2, int d, int h,
                         int e_base, int E_local, float* out, void* stream);

/* smoe_skip_gate_bwd: backward of one gated half of the residual-MoE block in TRAINING (models/resMoE.py:68-77: hard masks with
 * the straight-through estimator; 131-143: tk = xn * m1, skip_tk = xn * m0, out = f(tk) + tk + skip_tk).  xn [T,d] f32 = the normed
 * activations, g_f [T,d] (f32 / f16 / bf16) = d loss / d tk as the operator's input, g_out [T,d] f32 = d loss / d out (or NULL),
 * mask [T,2] f32 = the forward's decisions (skip, keep: smoe_gate_ln_router), gate_w [d], gate_b [1] or NULL.  One pass, p recomputed:
 *     dz[t]  = -<g_f[t], xn[t]> p (1 - p),  p = sigmoid(<xn[t], gate_w> + gate_b)          (d loss / d gate logit; f32 [T] or NULL)
 *     dxn[t] = g_f[t] * keep[t] + g_out[t] + dz[t] * gate_w                                 (f32 [T,d]: into the LayerNorm backward)
 * gate_on = 0 (Gate.disable: constant masks, no gradient): dxn = g_f + g_out, dz = 0.  d in {192, 384, 768, 1024}.
 * gate_on = 2 (the SOFT gate, Gate(is_hard=False) in training, resMoE.py:72-74: m1 = p, m0 = 1 - p; mask = smoe_soft_gate_ln_fwd's
 * (1 - p, p)):  dz[t] = +<g_f[t], xn[t]> p (1 - p)  (the opposite sign),  dxn[t] = g_f[t] * p[t] + g_out[t] + dz[t] * gate_w  (the same line,
 * keep = mask[t, 1] = p).  Every other value of gate_on is refused.
 * The gate's parameter gradients follow from dz: dW = dz^T xn (smoe_gate_wgrad with E = 1), db = sum dz.                      */
int smoe_skip_gate_bwd(const float* xn, const void* g_f, int g_f_dtype, const float* g_out, const float* gate_w,
                       const float* gate_b, const float* mask, int gate_on, int64_t T, int d, float* dxn, float* dz, void* stream);
/* smoe_gate_ln_bwd: smoe_skip_gate_bwd, the LayerNorm backward in front of it and the gate's parameter gradients as ONE pass over the
 * half's INPUT x [T,d] f32 (the normed activations, p and the gate logit are recomputed from x in registers; nothing but x and the
 * forward's decisions is read):  dx [T,d] f32 = LayerNorm backward of dxn;  out f32 [3 d + 4] = dgamma [d] | dbeta [d] | dgate_w [d] |
 * dgate_b, 0, 0, 0;  dz f32 [T] or NULL.  gamma / beta f32 [d] (NULL = 1 / 0); the other operands as in smoe_skip_gate_bwd; d % 4 == 0,
 * d <= 1024.  Deterministic (per-workgroup partial rows, two-stage ordered reduction).  gate_on = 0 / 1 / 2 as smoe_skip_gate_bwd.     */
size_t smoe_gate_ln_bwd_workspace_bytes(int64_t T, int d);
int smoe_gate_ln_bwd(const float* x, const void* g_f, int g_f_dtype, const float* g_out, const float* gamma, const float* beta,
                     float eps, const float* gate_w, const float* gate_b, const float* mask, int gate_on, int64_t T, int d, float* dx,
                     float* dz, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* smoe_soft_gate_ln_fwd: the front end of one gated half in TRAINING with a SOFT gate (Gate(is_hard=False), models/resMoE.py:72-74:
 * skip_tk = 1 - p, tk = p -- no decision, so no threshold and no f64 redo), ONE pass over x [T,d] f32:
 *   xn   = (with_ln & 1) ? LN(x) * gamma + beta : x                 (two-pass statistics; gamma / beta NULL = 1 / 0)
 *   z    = <xn, gate_w> + gate_b (NULL = 0);  e = exp(-|z|);  p = 1 / (1 + e) or e / (1 + e) by the sign of z, 1 - p the other one
 *   xn32 [T,d] f32: xn (the residual: out = f(tk) + xn);  tk32 [T,d] f32: xn * p, ONE f32 multiply;  tk16 [T,d] f16 / bf16: the
 *   conversion of that f32 product (smoe_gate_ln_router's xn16 conversion);  mask [T,2] f32 = (1 - p, p).  Each may be NULL.
 *   *skip_count (int32, may be NULL) += rint(sum_t (1 - p[t])), summed in double in a fixed order by a second one-wave launch from
 *   per-workgroup partial sums in `workspace` (8-byte aligned, smoe_soft_gate_ln_fwd_workspace_bytes(T); unused without a counter).
 *   A row whose 1 - p is NaN counts as 0.  No atomics, no host access: capturable.  The backward is smoe_gate_ln_bwd / smoe_skip_gate_bwd
 *   with gate_on = 2, which recompute this pass's xn and z bit for bit.
 * d in {192, 384, 768, 1024} (smoe_soft_gate_ln_fwd_supported), 0 <= T < 2^31 (T == 0 returns at once).                          */
int smoe_soft_gate_ln_fwd_supported(int d);
size_t smoe_soft_gate_ln_fwd_workspace_bytes(int64_t T);
int smoe_soft_gate_ln_fwd(const void* x, int x_dtype, int with_ln, const float* ln_gamma, const float* ln_beta, float ln_eps,
                          const float* gate_w, const float* gate_b, float* xn32, void* tk16, int tk16_dtype, float* tk32, float* mask,
                          int32_t* skip_count, int64_t T, int d, void* workspace, size_t workspace_bytes, void* stream);

/* smoe_depth_scale_rows: stochastic depth's per-sample factor (timm DropPath as models/vision_transformer.py:308 uses it: x / keep * mask)
 * expanded to the sample's rows, the form the fused stores take it in (the GEMM's per-row combine scale): mask f32 [B] (0 / 1 draws)
 * -> factor f32 [B] = mask / keep (IEEE division), rows f32 [B * N] = factor[row / N].                                                 */
int smoe_depth_scale_rows(const float* mask, float keep, int64_t B, int N, float* factor, float* rows, void* stream);
/* ---- the embedding stage and the last LayerNorm of the ViT forward (models/vision_transformer.py:818-830) ----
 * smoe_patchify_cast:  images f32 [B, C, H, W] -> patch rows [B * (H/ph) * (W/pw), C * ph * pw] (f16 / bf16), row (b, gy, gx) =
 *                      images[b, :, gy*ph:(gy+1)*ph, gx*pw:(gx+1)*pw] flattened (c, py, px) -- the operand of the per-patch projection
 *                      GEMM (timm PatchEmbed: Conv2d with kernel == stride); pw % 4 == 0
 * smoe_embed_ln:       x32[b, 0] = cls_token + pos_embed[0],  x32[b, n] = tokens[b * P + n - 1] + pos_embed[n]  (n = 1 .. P)  -- the
 *                      f32 residual stream [B, P + 1, d] -- and, when xn != NULL, xn = LayerNorm(x32) in f16 / bf16 (block 0's norm1)
 *                      from the same pass.  tokens [B * P, d] f16 / bf16 (the projection GEMM's output), cls_token [d], pos_embed
 *                      [P + 1, d], gamma / beta [d] f32; d in {192, 384, 768, 1024}
 * smoe_embed_ln2:      smoe_embed_ln with a second prefix row, the distillation token of DeiT's DistilledVisionTransformer
 *                      (models/model.py:48-67): x32[b, 0] = cls_token + pos_embed[0], x32[b, 1] = dist_token + pos_embed[1],
 *                      x32[b, n] = tokens[b * P + n - 2] + pos_embed[n] (n = 2 .. P + 1) -- the stream [B, P + 2, d], pos_embed
 *                      [P + 2, d] -- and the optional LayerNorm as above.  dist_token == NULL: one prefix row, the launch and the bits
 *                      of smoe_embed_ln.
 * smoe_layernorm_rows: LayerNorm of T f32 rows that start row_stride elements apart (the class-token rows x[:, 0] behind the last
 *                      block: row_stride = (P + 1) * d); out f32 [T, d]                                                              */
int smoe_patchify_cast(const float* images, int64_t B, int C, int H, int W, int ph, int pw, void* out, int out_dtype, void* stream);
int smoe_embed_ln(const void* tokens, int tok_dtype, const float* cls_token, const float* pos_embed, const float* ln_gamma,
                  const float* ln_beta, float ln_eps, int64_t B, int P, int d, float* x32, void* xn, int xn_dtype, void* stream);
int smoe_embed_ln2(const void* tokens, int tok_dtype, const float* cls_token, const float* dist_token, const float* pos_embed,
                   const float* ln_gamma, const float* ln_beta, float ln_eps, int64_t B, int P, int d, float* x32, void* xn, int xn_dtype,
                   void* stream);
int smoe_layernorm_rows(const float* x, int64_t row_stride, const float* gamma, const float* beta, float eps, int64_t T, int d,
                        float* out, void* stream);

/* LayerNorm alone (same arithmetic as the fused form; the `norm1` of models/vision_transformer.py:320 feeding the
 * attention GEMMs in 16 bit): d in {192, 384, 768, 1024}.                                              */
int smoe_layernorm(const void* x, int x_dtype, const float* gamma, const float* beta, float eps, int64_t T, int d,
                   void* out, int out_dtype, void* stream);

/* Self-attention forward of the block's attention half (models/vision_transformer.py:248-280), N <= 640 tokens
 * (one pass for N <= 256; above that -- ViT-L/16 @384: N = 577 -- key chunks with an online softmax),
 * head dim 64: out[b,n,h*64+:] = softmax(q k^T * scale) v with qkv [B,N,3,H,64] as the fused qkv projection
 * writes it; f16 / bf16.  Caller-side kernel, not part of the MoE operator.       */
int smoe_attention_supported(int N, int head_dim);
int smoe_attention_fwd(const void* qkv, void* out, int dtype, int B, int N, int H, int head_dim, float scale,
                       float* lse, void* stream);
/* lse (may be NULL): [B, H, N] f32, log2 of the softmax normaliser in the scaled-score domain, p = exp2(s scale
 * log2(e) - lse) -- what the backward recomputes the probabilities from.
 * smoe_attention_bwd: dqkv [B,N,3,H,64] (same fused layout) from qkv, the forward's out and lse, and dout [B,N,H*64]:
 * dV = P^T dO, dS = P (dO V^T - rowsum(dO O)) scale, dQ = dS K, dK = dS^T Q; scores recomputed per (image, head).  N <= 640
 * (smoe_attention_bwd_supported): one kernel with Q, K, V, dO whole in LDS for N <= 256; above that -- ViT-L/16 @384, N = 577,
 * models/vision_transformer.py:1227-1236 -- a dQ kernel (K / V in LDS, keys walked in chunks) and a dK / dV kernel (one
 * workgroup per 128-key block, Q / dO streamed) on the same stream, each finishing its outputs alone: no atomics, no
 * workspace, the same bits on every call.                                                                            */
int smoe_attention_bwd_supported(int N, int head_dim);
int smoe_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int dtype, int B, int N,
                       int H, int head_dim, float scale, void* stream);

/* ---- skip-aware attention half (eval; csrc/attention_skip.hip; additive to ABI 29) ------------------------------------------
 * With a hard dense_gate a bypassed token's operand row is exactly zero, so its q / k / v are the rounded qkv bias: per image with
 * n entering and m = N - n bypassed tokens the attention half needs n + 1 rows (n when m == 0) -- the m equal keys are one key
 * whose probability counts m times, the m equal queries one query whose projection row is added to every bypassed residual row.
 * Every entry point: no allocation, no synchronisation, no float atomics, the same bits on every call, capturable.
 *
 * smoe_skip_plan: mask f32 [B*N, 2] as smoe_gate_ln_router writes it (channel 0 > 0.5 = bypassed) -> all on the device,
 *   row_start / len / mult  i32 [B]: image b owns the compact rows [row_start[b], row_start[b] + len[b]), len = n_b + (m_b > 0),
 *                           mult = m_b; row_start is the running sum of len
 *   gather   i64 [B*N]      compact row -> token row: the entering tokens of image 0 in token order, then image 0's FIRST bypassed
 *                           token as its representative (if m_0 > 0), then image 1, ...; R = sum len <= B*N rows are in use
 *   row_map  i64 [B*N]      compact row -> output row of the projection: the token row, or B*N + b for image b's representative
 *   offsets  i32 [2]        {0, R}: the one row group of both GEMMs
 *   rep_row  i32 [B*N]      per token: B*N + b for a bypassed token of image b, -1 for an entering one
 *   entries of gather / row_map at and past R belong to no row group; they are set to 0 / B*N.
 *   park (may be NULL): f32 [B, park_cols], zeroed -- the B rows behind the token matrix that hold the representatives' outputs
 *   (the projection adds its `residual` row, which must be zero there).  B*N + B < 2^31.
 * smoe_attention_fwd_varlen: smoe_attention_fwd's one-pass forward over the compact qkv [rows_cap, 3, H, 64] -> out [rows_cap, H*64]
 *   (the same compact rows), one workgroup per (image, head); rows and key count of image b from row_start / len, and with
 *   mult[b] > 0 the image's LAST key counts mult[b] times.  max_len (host-side bound on len, <= 256) picks the instantiation; an image
 *   whose plan entry does not fit (len < 1, len > max_len rounded up to the instantiation, rows outside [0, rows_cap)) is left
 *   unwritten.  flags: SMOE_VARLEN_WEIGHT_SCORE = log2(mult) is added to the last key's scaled score instead of multiplying its
 *   probability (default: the probability, exact for an integer); SMOE_VARLEN_NO_TIERS = every image walks the key-tile count of
 *   max_len (default: an image takes the smallest of 4 / 8 / 13 / 16 tiles that holds its len).  f16 / bf16, head dim 64.
 * smoe_skip_expand: out[t, :] = xn32[t, :] + out[rep_row[t], :] for every t < T with rep_row[t] >= 0; other rows untouched.  xn32 may
 *   be out itself.  f32, d % 4 == 0, out_rows = rows allocated in out (rep_row values at or past it are ignored).           */
enum { SMOE_VARLEN_WEIGHT_SCORE = 1, SMOE_VARLEN_NO_TIERS = 2 };
int smoe_skip_plan(const float* mask, int B, int N, int32_t* row_start, int32_t* len, int32_t* mult, int64_t* gather,
                   int64_t* row_map, int32_t* offsets, int32_t* rep_row, float* park, int park_cols, void* stream);
int smoe_attention_fwd_varlen(const void* qkv, void* out, int dtype, const int32_t* row_start, const int32_t* len,
                              const int32_t* mult, int B, int max_len, int64_t rows_cap, int H, int head_dim, float scale,
                              int flags, void* stream);
int smoe_skip_expand(const float* xn32, const int32_t* rep_row, float* out, int64_t T, int d, int64_t out_rows, void* stream);

/* ---- dispatch plan --------------------------------------------------------------------------------
 * Replaces fmoe_cuda.expert_count + cumsum + assign_pos (+ limit_by_capacity /
 * prune_gate_by_capacity) = fmoe count_by_gate / prepare_forward.
 * Deterministic stable counting sort of the n = T*k flat entries by expert id:
 *   counts[e]  = kept entries on e (min(raw, capacity) when capacity >= 0)
 *   offsets    = exclusive prefix of counts, offsets[E] = kept total
 *   pos[s]     = flat index t*k+j of slot s (ascending flat index inside an expert); -1 for s >= kept
 *   inv_pos[i] = slot of flat entry i, -1 if dropped (idx < 0 or over capacity)
 *   idx_pruned = idx with dropped entries set to -1 (may be NULL when capacity < 0)
 * idx values must lie in [-1, E).  workspace: smoe_dispatch_plan_workspace_bytes(n, E) bytes.   */
size_t smoe_dispatch_plan_workspace_bytes(int64_t n, int E);
int smoe_dispatch_plan(const int64_t* idx, int64_t n, int E, int64_t capacity,
                       int32_t* counts, int32_t* offsets, int64_t* pos, int64_t* inv_pos,
                       int64_t* idx_pruned, void* workspace, size_t workspace_bytes, void* stream);
/* smoe_dispatch_plan_subset: the plan over a PERIODIC SUBSET of the flat entries -- entry i is dispatched iff i % period < prefix
 * (0 <= prefix <= period < 2^31; for "the first p of every P tokens" of a top-k pass: period = P * k, prefix = p * k).  Every other
 * entry is read as -1: counts / offsets / pos are the full plan restricted to the dispatched entries, in the same stable order
 * (expert, then flat index); pos[s] and inv_pos[i] keep numbering the entries of the FULL idx (what smoe_grouped_gemm's a_gather /
 * row_map take: no compacted copy of tokens, idx or scores exists), pos[s] = -1 for s >= offsets[E], inv_pos[i] = -1 for an entry
 * that is not dispatched.  idx = -1 keeps its meaning, empty groups are ordinary.  No capacity (a capacity rank is defined over all
 * entries).  period == 0: every entry -- bit for bit smoe_dispatch_plan(capacity = -1).  Same workspace.  What it is for: the last
 * block of an eval forward, whose classifier reads the class-token rows only (vit.VisionTransformer.tail_rows_only). */
int smoe_dispatch_plan_subset(const int64_t* idx, int64_t n, int E, int64_t period, int64_t prefix, int32_t* counts,
                              int32_t* offsets, int64_t* pos, int64_t* inv_pos, void* workspace, size_t workspace_bytes,
                              void* stream);
/* smoe_dispatch_plan_hist: the same plan from a chunk histogram the fused router wrote (smoe_ln_router_topk / smoe_gate_ln_router
 * `chunk_hist`; hist_chunk = tokens per row x k flat entries): one launch, no counting pass over idx.  Falls back to
 * smoe_dispatch_plan when the table does not fit the fused kernel.  idx here is what the plan is built over (for the gated MoE
 * half: idx_plan, -1 = not dispatched -- exactly the entries the router left out of the histogram).                          */
int smoe_dispatch_plan_hist(const int64_t* idx, int64_t n, int E, int64_t capacity, const int32_t* hist, int hist_chunk,
                            int32_t* counts, int32_t* offsets, int64_t* pos, int64_t* inv_pos, int64_t* idx_pruned,
                            void* workspace, size_t workspace_bytes, void* stream);
/* The same plan in the PADDED layout of a capacity gate's static expert-parallel exchange (SURVEY.md section 8e, Appendix B
 * `cap` note: "[W, E_local, cap, d] exchange buffers, no count exchange / host sync needed"): expert e owns the slots
 * [e * slot_rows, (e + 1) * slot_rows) whatever its count, slot = e * slot_rows + rank (slot_rows >= capacity: the slot
 * size every rank agreed on, e.g. the capacity of the largest local batch; `capacity` is what THIS rank keeps).  pos_padded
 * has E * slot_rows entries (unused slots -1), inv_pos[i] is the padded slot, group_end[e] = e * slot_rows + counts[e] closes
 * expert e's row range (smoe_grouped_gemm's `group_end`); counts / offsets as above.  capacity >= 1; E <= 64. */
int smoe_dispatch_plan_padded(const int64_t* idx, int64_t n, int E, int64_t capacity, int64_t slot_rows, int32_t* counts,
                              int32_t* offsets, int32_t* group_end, int64_t* pos_padded, int64_t* inv_pos,
                              int64_t* idx_pruned,
                              int32_t* raw_counts /* i32 [E] or NULL: entries routed to each expert BEFORE the capacity clamp */,
                              void* workspace, size_t workspace_bytes, void* stream);

/* The same plan over a SLOT TABLE (the static expert exchange's send layout): expert e owns the slots [slot_base[e],
 * slot_base[e + 1]) (slot_base i32 [E + 1], device memory), the last hdr_rows (0 / 1) of them reserved for the in-band header; it
 * keeps min(region - hdr_rows, capacity if capacity >= 0) entries.  pos_slots has slot_base[E] entries (unused ones -1), inv_pos[i]
 * is the slot, group_end[e] = slot_base[e] + counts[e]; raw_counts as above.  E <= 64. */
int smoe_dispatch_plan_slots(const int64_t* idx, int64_t n, int E, int64_t capacity, const int32_t* slot_base, int hdr_rows,
                             int32_t* counts, int32_t* offsets, int32_t* group_end, int64_t* pos_slots, int64_t* inv_pos,
                             int64_t* idx_pruned, int32_t* raw_counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- in-band headers of the static expert exchange ------------------------------------------------------------------------
 * Replaces fmoe_cuda.expert_exchange (the count all-to-all in front of global_scatter) for the static exchange:
 * the counts travel INSIDE the token all-to-all.  Send buffer = one region per global expert g, rows [slot_base[g],
 * slot_base[g + 1]) (blocks of E_local consecutive regions go to one peer): payload rows + ONE header row (the region's last),
 * whose leading int32 words are {kept rows of the group, rows routed to it before the clamp, the source's row count, G, the
 * source's pre-clamp counts of ALL G experts}.  row_bytes >= 16 + 4 G.
 * smoe_ep_pack_headers writes the G header rows of a send buffer (counts / raw_counts i32 [G] from smoe_dispatch_plan_slots;
 * raw_counts NULL = counts; counts NULL = a rank without rows);
 * smoe_ep_unpack_headers reads the W * E_local headers of a RECEIVED buffer ([source rank][local expert] order; local_base i32
 * [E_local + 1] = this rank's experts' region offsets inside one source's block, local_base[E_local] = rows per block):
 *   starts[l], ends[l] (i32 [W * E_local])  -> smoe_grouped_gemm's offsets / group_end
 *   stats (may be NULL) i32 [W][1 + E_total] = {source w's row count, source w's pre-clamp counts of all experts} -- every rank
 *   receives the same matrix, so all ranks can decide "somebody overflowed" (and re-size the slots) identically, without a collective */
int smoe_ep_pack_headers(const int32_t* counts, const int32_t* raw_counts, const int32_t* slot_base, int G, int64_t row_bytes,
                         int64_t t_rows, void* send, void* stream);
int smoe_ep_unpack_headers(const void* recv, int W, int E_local, const int32_t* local_base, int64_t row_bytes, int E_total,
                           int32_t* starts, int32_t* ends, int32_t* stats, void* stream);

/* ---- token scatter (MOEScatter.forward local part: index_select(x, 0, pos // k)) ----
 * buf[s,:] = cast(x[pos[s] / k, :]) for every slot s < n_slots with pos[s] >= 0; other rows untouched.
 * x [T,d], buf [n_slots,d]; d % 8 == 0.  scale (f32 [T*k], may be NULL) multiplies row s by scale[pos[s]]
 * (backward of the combine: dY[s] = score * dout[token]).                                           */
int smoe_scatter_rows(const void* x, int x_dtype, const int64_t* pos, const float* scale, int64_t n_slots, int k, int d,
                      void* buf, int buf_dtype, void* stream);
/* the same, and every slot with pos[s] < 0 (no token: past the kept count under a capacity) is written as a zero row in the same
 * pass (the training path's buffers: instead of clearing the whole buffer first).                                             */
int smoe_scatter_rows_fill(const void* x, int x_dtype, const int64_t* pos, const float* scale, int64_t n_slots, int k, int d,
                           void* buf, int buf_dtype, void* stream);

/* ---- gather + combine (MOEGather.forward + bmm(gate_score, y)) -------------------
 * out[t,:] = sum_j score[t,j] * y[inv_pos[t*k+j], :]   (a dropped entry contributes 0)
 * optional fused residual add (the `+ tk + skip_tk` of models/resMoE.py:143): out[t,:] += residual[t,:]
 * when residual != NULL (same dtype as out).  y [n_slots,d] (y_dtype), out [T,d] (out_dtype).       */
int smoe_gather_combine(const void* y, int y_dtype, const int64_t* inv_pos, const float* score,
                        int64_t T, int k, int d, const void* residual, void* out, int out_dtype,
                        void* stream);
/* smoe_gather_combine_ln: the same combine (+ residual, f32 out [T,d]) AND LayerNorm(out row) -> xn [T,d] (f16 / bf16) in one pass:
 * the next block's `norm1` of exactly the row this call produces (models/vision_transformer.py:320) -- the expert-parallel
 * return path saves a 155-MB read per layer.  y f16 / bf16; k <= 4; d % 8 == 0, d <= 1024; gamma / beta f32 [d].             */
int smoe_gather_combine_ln(const void* y, int y_dtype, const int64_t* inv_pos, const float* score, int64_t T, int k, int d,
                           const float* residual, float* out, const float* gamma, const float* beta, float eps, void* xn,
                           int xn_dtype, void* stream);

/* ---- grouped (variable-batch) expert GEMM on MFMA ----------------------------------------------------
 * Replaces fmoe_cuda.linear_forward = MOELinear / FMoELinear: for each local
 * expert e, rows r in [offsets[e], offsets[e+1]):
 *     out[r, :] = epilogue( A[r, :] @ W[e]^T + bias[e] )          W [E,N,K] row-major ([out,in])
 * One launch for all experts; the tile -> (expert, m-tile) map is derived on device from `offsets`
 * (no host sync; empty experts are fine).  m_rows_max = upper bound on offsets[E] (rows allocated in A/out).
 * ab_dtype: SMOE_F16 / SMOE_BF16 (MFMA 16-bit inputs, f32 accumulate) or SMOE_F32 (exact f32 MFMA).
 * bias f32 [E,N] or NULL.  epilogue SMOE_EPI_GELU = exact-erf GELU (models/resMoE.py:23-25).
 * Optional fused combine for top-1 (row_map != NULL): row r is stored to out[row_map[r], :]
 * multiplied by row_scale[row_map[r]] if row_scale != NULL  (MOEGather + bmm for k = 1).
 * Optional fused residual (residual != NULL, same dtype / shape as out): the stored value is
 * residual[orow, :] + value -- the `x + mlp(norm2(x))` add of models/vision_transformer.py:321.
 * Optional fused scatter (a_gather != NULL; variants 4-14): row r of the GEMM reads A[a_gather[r] / a_div, :]
 * instead of A[r, :] -- MOEScatter's index_select(x, pos // k) folded into the operand DMA (A = the token matrix).
 * The library never learns how many rows that A has (m_rows_max counts the gathered rows): with a_gather the persistent
 * variants 9-14 need ALL of A under 4 GiB -- the caller's duty; their 32-bit byte offsets would otherwise read rows modulo 2^32
 * with no error.  Variants 4-8 hold 64-bit row pointers and take any A (the Python wrapper sends a larger A there).
 * SMOE_EPI_GELU_GRAD (backward of the activation, fused into the dgrad GEMM): `residual` then holds the saved
 * pre-activations H and the stored value is value * gelu'(H[r, :]).
 * Optional group -> expert map (group_expert != NULL, i32 [G]): `offsets` then delimits G row groups and
 * group g uses W[group_expert[g]] / bias[group_expert[g]] (expert-parallel receive layout: one group per
 * (source rank, local expert)); n_experts = leading dimension of W / bias.
 * Optional separate row ranges (group_end != NULL, i32 [G]; persistent kernel only): group g is the rows
 * [offsets[g], group_end[g]) and `offsets` holds G entries -- the padded [W, E_local, cap] receive buffer of a capacity
 * gate's static exchange, whose slots are only partly filled (smoe_dispatch_plan_padded); tiles past a group's end are
 * never scheduled, so the padding costs no MFMA work.
 * out_rows = rows allocated in `out` (and `residual`): every row_map value must be below it.  0 = not stated (taken as
 * m_rows_max without a row map); the persistent kernel then keeps flat addressing for f32 outputs instead of the
 * buffer-addressed epilogue (whose descriptors need the bound: out_rows * N * 4 < 2 GiB).
 * Requires K*sizeof(ab) % 128 == 0 and N % 8 == 0.
 * variant: 4-14 are a table of kernel family x tile plan, every entry a 256-column tile on the 8-wave ping-pong structure with
 * LDS-DMA staging:                                  auto   320-row   256-row   256-row deep   320-row deep
 *   one workgroup per tile                            4       5         6           7              8
 *   persistent (one workgroup per CU walks tiles)     9      10        11          12             13
 * auto = the tile rule smoe_grouped_gemm_plan states; deep = the deep prefetch schedule.  9 = production choice: the persistent
 * family stores plain 16-bit outputs from the registers and f32 outputs through buffer descriptors; 14 = 9 with the LDS-staged
 * epilogue everywhere (A/B reference).  A persistent variant whose operands reach 4 GiB, or with more than 63 groups, runs the
 * same plan in the one-workgroup-per-tile family.  1-3 earlier LDS-DMA structures and 0 the register-staged kernel (the only
 * one for f32 operands or K % 64 != 0; chosen automatically then) are kept as A/B references.
 * All variants compute the same function.                                                              */
int smoe_grouped_gemm(const void* A, const void* W, const float* bias, const int32_t* offsets,
                      const int32_t* group_expert, int G, int n_experts, int64_t m_rows_max, int K, int N,
                      int ab_dtype, int epilogue, const int64_t* row_map, const float* row_scale,
                      const void* residual, const int64_t* a_gather, int a_div,
                      void* out, int64_t out_rows, int out_dtype, int variant, const int32_t* group_end, void* stream);
/* The tile rule of the auto variants (4, 9, 14) for `rows` rows in G groups on the current device, as the explicit persistent
 * variant it resolves to (10-13), for callers that name the variant from host-side numbers of their own:
 *   t(h) = (ceil(rows / h) + G / 2) * ceil(N / 256) expected tiles of h rows (G / 2 rounds down), cus = the device's CU count;
 *   320-row tiles iff ceil(t(320) / cus) * 1.25 <= ceil(t(256) / cus) (ties go to the taller tile); deep schedule iff K >= 2048. */
int smoe_grouped_gemm_plan(int64_t rows, int G, int K, int N);

/* OPTIONAL -- only in a library built with `make FFN=-DSMOE_FFN_FUSED` (it measured slower than the two smoe_grouped_gemm launches in
 * every scheduler design, profiles/r04_fused_ffn.md, and left the default build in round 5; bit-identical to them).
 * smoe_expert_ffn: the whole expert FFN of one MoE layer with the top-1 combine -- fmoe_cuda.linear_forward x 2 with the activation
 * between them, MOEGather and the combine (models/resMoE.py:143 -> FastMoE `_Expert.forward`) -- as ONE persistent
 * launch:   H[r]   = gelu(X[a_gather[r] / a_div] W1[e]^T + b1[e])                      (16-bit, [m_rows_max, d_hidden]; caller's buffer)
 *           out[row_map[r]] = residual[row_map[r]] + row_scale[row_map[r]] (H[r] W2[e]^T + b2[e])       (f32, [out_rows, d_out])
 * for r in row group g's range [offsets[g], offsets[g+1]), e = group_expert[g] (or g).  Every number is computed exactly as by the
 * two smoe_grouped_gemm launches (variant 9: 320-row tiles, same accumulation order): bit-identical results.  What the single
 * launch buys: the workgroups draw tiles of BOTH GEMMs from one list (a GEMM-2 tile starts when the GEMM-1 tiles of its rows
 * have stored, counted per m-tile in `workspace`), so neither GEMM ends in a partly filled round of workgroups.
 * a_gather / row_map / row_scale / residual / b1 / b2 / group_expert may be NULL.  `workspace`: smoe_expert_ffn_workspace_bytes
 * bytes, ZERO before the first launch; every launch leaves it zero again (word 17 = error flag: set if a wait on a row counter ran
 * out -- never in a healthy launch).  Returns -1 (no error set) for shapes outside this launch's reach (operands not f16 / bf16,
 * out not f32, d_in or d_hidden % 64, > 63 groups, operands >= 4 GiB, out >= 2 GiB): issue the two smoe_grouped_gemm then.
 * With a_gather ALL of X must be under 4 GiB (the caller's duty, as for smoe_grouped_gemm's variants 9-14: the row count of X is
 * not an argument). */
size_t smoe_expert_ffn_workspace_bytes(int64_t m_rows_max, int G);
int smoe_expert_ffn(const void* X, const int64_t* a_gather, int a_div, const void* W1, const float* b1, void* H, const void* W2,
                    const float* b2, const int32_t* offsets, const int32_t* group_expert, int G, int n_experts,
                    int64_t m_rows_max, int d_in, int d_hidden, int d_out, int ab_dtype, const int64_t* row_map,
                    const float* row_scale, const void* residual, void* out, int64_t out_rows, int out_dtype, void* workspace,
                    size_t workspace_bytes, void* stream);

/* smoe_grouped_gemm_gelu_keep: the first expert linear of the TRAINING forward (fmoe_cuda.linear_forward + the activation, whose
 * input autograd keeps): pre_out = A W^T + bias and out = gelu(pre_out), both [m_rows, N] in the operand dtype (f16 / bf16), from one
 * epilogue.  Returns -1 (no error set) for shapes outside the persistent kernel's reach (K % 64 != 0, operands >= 4 GiB, G > 63):
 * use smoe_grouped_gemm(SMOE_EPI_NONE) + smoe_gelu then.  group_end (optional, i32 [G]): separate row ranges [offsets[g], group_end[g])
 * as in smoe_grouped_gemm -- the slots of the static expert exchange in training; rows outside the ranges are neither read nor written. */
int smoe_grouped_gemm_gelu_keep(const void* A, const void* W, const float* bias, const int32_t* offsets,
                                const int32_t* group_expert, const int32_t* group_end, int G, int n_experts, int64_t m_rows_max,
                                int K, int N, int ab_dtype, void* pre_out, void* out, void* stream);

/* ---- backward pieces (fmoe_cuda.linear_backward and the adjoints of scatter / gather) ---------
 * smoe_gelu:            dst = gelu_erf(src), n % 8 == 0 (training forward keeps the pre-activations)
 * smoe_rowdot:          dscore[i] = <dout[i / k, :], y[inv_pos[i], :]>, 0 for dropped entries (i < n = T*k)
 * smoe_pad_offsets:     offsets_pad[e] = sum_{e'<e} round_up(count[e'], 64)
 * smoe_transpose_pad:   src [n_rows, C] expert-sorted -> dst [C, Lp] K-major, per-expert ranges at offsets_pad, zero pad
 * smoe_grouped_wgrad:   out[e] (f32 [R1,R2]) = PT[:, range e] @ QT[:, range e]^T   (PT [R1,Lp], QT [R2,Lp], 16-bit)
 * smoe_group_colsum:    out[e, c] = sum over expert e's rows of src[:, c]  (bias gradients); C % 4 == 0; two passes
 *                       (512-row chunk partials in `workspace`, then a per-expert sum in chunk order: deterministic);
 *                       n_rows_max >= offsets[E] sizes the launch; group_end (optional, i32 [E]): expert e's rows are
 *                       [offsets[e], group_end[e]) -- separate ranges (slots of the static expert exchange), n_rows_max >=
 *                       the sum of their lengths                                                                        */
int smoe_gelu(const void* src, void* dst, int dtype, int64_t n, void* stream);
int smoe_rowdot(const void* dout, int dout_dtype, const void* y, int y_dtype, const int64_t* inv_pos,
                int64_t n, int k, int d, float* dscore, void* stream);
int smoe_pad_offsets(const int32_t* offsets, int E, int32_t* offsets_pad, void* stream);
/* smoe_split_offsets: every row group [offsets[g], offsets[g + 1]) cut into S pseudo-groups of whole 64-row chunks (the last ones may be
 * empty): out i32 [G * S + 1].  smoe_grouped_wgrad_rows' grid is groups x output tiles, so a weight gradient over few long groups
 * (fmoe_cuda.linear_backward's grad_W at DeiT-Tiny's dims: 24 tiles) is computed as S partial products per expert, summed in piece
 * order by the caller (deterministic). */
int smoe_split_offsets(const int32_t* offsets, int G, int S, int32_t* out, void* stream);
int smoe_transpose_pad(const void* src, int dtype, const int32_t* offsets, const int32_t* offsets_pad, int E,
                       int64_t n_rows, int C, int Lp, void* dst, void* stream);
/* smoe_switch_gate_bwd: gradient of the SwitchGate's score and load-balance loss w.r.t. the router logits (fmoe.gates.SwitchGate:
 * score = softmax(logits)[idx], aux = E sum_e frac_e prob_e), one pass over [T, E]:  g[t,e] = coef[e] + (e == idx[t] ? dscore[t] : 0),
 * dlogits[t,e] = probs[t,e] (g[t,e] - sum_j probs[t,j] g[t,j]).  coef [E] f32 (device; = E * frac_e / kept, smoe_switch_aux's) or
 * NULL, times *coef_scale (device scalar: d loss / d aux; NULL = 1); dscore [T] f32 or NULL, idx [T] int64 (entries outside
 * [0, E) select nothing).                                                                                                       */
int smoe_switch_gate_bwd(const float* probs, const int64_t* idx, const float* dscore, const float* coef, const float* coef_scale,
                         int64_t T, int E, float* dlogits, void* stream);
/* smoe_switch_aux: the SwitchGate's load-balance loss (fmoe.gates.SwitchGate), forward: aux [1] = E sum_e frac_e prob_e,
 * frac_e = counts[e] / kept, prob_e = sum_t probs[t,e] / kept, kept = max(sum_e counts[e], 1); coef [E] = E frac_e / kept
 * (= d aux / d probs[t,e] for every t: what smoe_switch_gate_bwd takes).  probs f32 [T, E], counts i32 [E] (the plan's kept counts);
 * E <= 256; two deterministic launches (chunk column sums, then one workgroup).                                                 */
size_t smoe_switch_aux_workspace_bytes(int64_t T, int E);
int smoe_switch_aux(const float* probs, const int32_t* counts, int64_t T, int E, float* aux, float* coef, void* workspace,
                    size_t workspace_bytes, void* stream);
/* GShard gate (fmoe.gates.GShardGate; the rule is restated in INTEGRATION.md), behind the NAIVE top-2 router.  E <= 256.
 * smoe_gshard_prune: idx int64 [T, 2] (the router's; ids outside [0, E) read as -1), score f32 [T, 2], u f32 [T] or NULL ->
 *   idx_out int64 [T, 2] and top1_counts i32 [E] = #{t : idx[t, 0] == e}.  Capacity first, in flat order: entry i = 2 t + j is kept
 *   while fewer than `capacity` entries i' < i named the same expert (capacity < 0: no clamp); then random routing: a second choice
 *   with 2 score[t, 1] < u[t] (f32 compare) becomes -1 and has still used its capacity slot.  Two launches (chunk histograms; ranks
 *   by wave ballots), deterministic.  ceil(2 T / 1024) * E <= 2^20.
 * smoe_gshard_aux: logits f32 [T, E] -> aux [1] = mean_e(c_e m_e) num_expert^2 with c_e = top1_counts[e] / T and
 *   m_e = mean_t softmax(logits[t, :])[e] (f32), and coef [E] = num_expert^2 top1_counts[e] / (E T^2) = d aux / d softmax[t, e] for
 *   every t.  num_expert = the local expert count (it divides E).  Two launches: column sums per 256-row chunk, then one workgroup
 *   adds the chunks in order -- no float atomics, bit-reproducible.
 * smoe_gshard_gate_bwd: one pass, p = softmax(logits[t, :]) recomputed:
 *   dlogits[t, e] = s p[e] (coef[e] - sum_j p[j] coef[j]) + [e == idx[t, a]] score_a (ds_a - (score_0 ds_0 + score_1 ds_1)), a = 0, 1,
 *   s = *coef_scale (device scalar: d loss / d aux; NULL = 1), coef NULL = no balance-loss term, ds_a = dscore[t, a], taken as 0 where
 *   idx_out[t, a] < 0 (whatever the buffer holds) and everywhere when dscore is NULL.                                            */
size_t smoe_gshard_prune_workspace_bytes(int64_t T, int E);
int smoe_gshard_prune(const int64_t* idx, const float* score, const float* u, int64_t T, int E, int64_t capacity, int64_t* idx_out,
                      int32_t* top1_counts, void* workspace, size_t workspace_bytes, void* stream);
size_t smoe_gshard_aux_workspace_bytes(int64_t T, int E);
int smoe_gshard_aux(const float* logits, const int32_t* top1_counts, int64_t T, int E, int num_expert, float* aux, float* coef,
                    void* workspace, size_t workspace_bytes, void* stream);
int smoe_gshard_gate_bwd(const float* logits, const int64_t* idx, const int64_t* idx_out, const float* score, const float* dscore,
                         const float* coef, const float* coef_scale, int64_t T, int E, float* dlogits, void* stream);
/* Noisy top-k gate (fmoe.gates.NoisyGate; the rule is restated in INTEGRATION.md), behind the router run over the [2E, d] image
 * [w_gate^T ; w_noise^T].  2 <= E <= 32, 1 <= k <= 4, k < E, ceil(T / 256) <= 2^24; anything else is refused before any launch.
 * smoe_noisy_gate_fwd: logits2 f32 [T, 2E] (columns 0..E-1 clean, E..2E-1 raw), eps f32 [T, E] or NULL (= zero noise) ->
 *   sigma = softplus(raw) + 1e-2 (torch's softplus: beta 1, threshold 20) when `training`, else 0; noisy = clean + eps sigma;
 *   v_1 >= .. >= v_{k+1} the k + 1 largest noisy values of the row at experts i_1 .. i_{k+1} (ties -> lowest id; a NaN is never
 *   chosen, and every id written lies in [0, E));  idx int64 [T, k] = (i_1 .. i_k), score f32 [T, k] = softmax(v_1 .. v_k),
 *   keep f64 [T, 2] = (v_k, v_{k+1}), next i32 [T] = i_{k+1};  imp [E] = the scores summed at their experts,
 *   load [E] = sum_t Phi((clean - thr) / sigma), thr = v_{k+1} where noisy > v_{k+1} (strict) else v_k (training; zeros in eval),
 *   aux [1] = cv2(imp) + cv2(load), cv2(v) = var_unbiased(v) / (mean(v)^2 + 1e-10), coef_imp / coef_load [E] = d aux / d imp_e,
 *   d aux / d load_e.  Two launches: a row pass leaving column partials per 256-row chunk, a finish pass adding them in chunk
 *   order -- no float atomics, bit-reproducible.  The arithmetic between the f32 inputs and outputs is f64.
 * smoe_noisy_gate_bwd: one pass (the scores are recomputed from the kept values' experts) -> dlogits2 f32 [T, 2E] of sum(score dscore) + *coef_scale aux.  dscore f32 [T, k] or NULL (no score
 *   term); coef_scale (device scalar, d loss / d aux) NULL = the loss is not in the objective: both loss terms are left out.   */
size_t smoe_noisy_gate_workspace_bytes(int64_t T, int E);
int smoe_noisy_gate_fwd(const float* logits2, const float* eps, int64_t T, int E, int k, int training, int64_t* idx, float* score,
                        double* keep, int32_t* next, float* imp, float* load, float* aux, float* coef_imp, float* coef_load,
                        void* workspace, size_t workspace_bytes, void* stream);
int smoe_noisy_gate_bwd(const float* logits2, const float* eps, const int64_t* idx, const double* keep, const int32_t* next,
                        const float* dscore, const float* coef_imp, const float* coef_load,
                        const float* coef_scale, int64_t T, int E, int k, int training, float* dlogits2, void* stream);
/* smoe_transpose_cast: dst[b][c][r] = (dst_dtype) src[b][r][c] for b < B; R % 64 == 0, C % 64 == 0.  The backward pass reads every
 * expert weight [E, out, in] a second time as [E, in, out] (FastMoE: `MOELinear.backward` -> fmoe_cuda.linear_backward contracts
 * grad_out with the weight over `out`); this makes that 16-bit image straight from the f32 master in one pass.               */
int smoe_transpose_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int B, int R, int C, void* stream);
int smoe_grouped_wgrad(const void* PT, const void* QT, int ab_dtype, const int32_t* offsets_pad, int E, int R1,
                       int R2, int Lp, float* out, void* stream);
/* smoe_grouped_wgrad_rows: the same weight gradients as smoe_grouped_wgrad, straight from the token-major operands
 * (P [n_rows,R1], Q [n_rows,R2], f16 / bf16, expert-sorted rows; offsets i32 [E+1] = plain row ranges, any lengths):
 * out[e] (f32 [R1,R2]) = sum_{r in expert e} P[r,:]^T Q[r,:].  No transposed copies: the MFMA fragments are read
 * from LDS with transposing reads.  R1, R2 multiples of 8; zero16 = 16 zero bytes in device memory.  group_end (optional, i32 [E]):
 * expert e's rows are [offsets[e], group_end[e]) -- separate ranges; nothing behind group_end[e] is read. */
int smoe_grouped_wgrad_rows(const void* P, const void* Q, int ab_dtype, const int32_t* offsets, const int32_t* group_end, int E,
                            int R1, int R2, const void* zero16, float* out, void* stream);
/* smoe_gate_wgrad: router weight gradient dWg [E, C] f32 = dl^T x, dl [n_rows, E] f32 (d loss / d logits), x [n_rows, C]
 * f32 / f16 / bf16; E <= 16, C % 4 == 0; HBM-bound two-pass weighted column sum (what torch's matmul backward of the gate
 * nn.Linear computes, models/resmoe_flop_hook.py:7-8 names that layer).  db (f32 [E], may be NULL) = column sums of dl, the gate
 * bias' gradient, from the same pass (x's "ones column"). */
size_t smoe_gate_wgrad_workspace_bytes(int64_t n_rows, int E, int C);
int smoe_gate_wgrad(const float* dl, const void* x, int x_dtype, int64_t n_rows, int E, int C, float* out, float* db,
                    void* workspace, size_t workspace_bytes, void* stream);
/* smoe_zero_group_fold: the training path's zero-row groups (tokens the token-skip gate masked, models/resMoE.py:141 `x * mask`: all-zero
 * rows, every one routed by the gate bias alone to expert gmap[E + j]) need no weight-gradient GEMM: group E + j adds the rank-1 term
 * colsum(dY_g) (x) A_row to dW2[gmap[E + j]] (the rows of A = gelu(b1[e]) are identical), and an expert's bias gradients are the column sums
 * of its own group plus those of the zero groups that use it.  cs2 f32 [E + Z, d], cs1 f32 [E + Z, h] = smoe_group_colsum of dY / dH over
 * all E + Z groups; A [n_rows, h] f16 / bf16 / f32; offsets i32 [E + Z + 1]; gmap i32 [E + Z]; dW2 f32 [E, d, h] updated IN PLACE;
 * db2 f32 [E, d], db1 f32 [E, h] written (either may be NULL).  h % 4 == 0.  Groups are folded in index order.                        */
int smoe_zero_group_fold(const float* cs2, const float* cs1, const void* A, int a_dtype, const int32_t* offsets, const int32_t* gmap,
                         int E, int Z, int d, int h, int64_t n_rows, float* dW2, float* db2, float* db1, void* stream);
size_t smoe_group_colsum_workspace_bytes(int64_t n_rows_max, int E, int C);
int smoe_group_colsum(const void* src, int dtype, const int32_t* offsets, const int32_t* group_end, int E, int64_t n_rows_max, int C,
                      float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- expert exchange (expert parallelism over RCCL / xGMI) ----------------------------------------------------------
 * Replaces fmoe_cuda.ensure_nccl / expert_exchange / global_scatter / global_gather (reached from
 * models/resMoE.py:27-29 when world_size > 1).  A context owns ONE RCCL communicator (built from a unique-id blob that
 * rank 0 creates with smoe_unique_id and the caller distributes by whatever means it has -- MPI, a file, torch's store),
 * ONE communication stream and a ring of completion events.  Every exchange is enqueued on the context's stream behind an
 * event recorded on the caller's `stream` (so it sees the send buffer the compute stream produced) and ends with an event
 * the caller's stream waits on: immediately when wait != 0, or later -- in between the compute stream is free to run other
 * work (the expert GEMMs of another micro-batch) while rows move over xGMI.  Every exchange has a ticket (1, 2, ...:
 * smoe_a2a_last_ticket right after posting it); smoe_a2a_wait_ticket waits for THAT exchange (the ring holds the last 16;
 * an older ticket waits for the exchange that re-used its slot, which is later on the same in-order stream), so exchanges
 * of several micro-batches in flight can be waited for in any order; smoe_a2a_wait = the latest one.  Arguments are
 * checked before the RCCL group opens and a failing call inside the group closes it before returning.  All peers' transfers of one
 * call are posted as one RCCL group: on the point-to-point xGMI mesh every link then carries its pair's rows concurrently.
 * RCCL is resolved at run time from the librccl.so already in the process (or the system's): no link-time dependency.
 *   smoe_a2a_counts : send_counts[w*E_local + e] = rows this rank routes to rank w's local expert e  ->  recv_counts[w*E_local
 *                     + e] = rows rank w routes to this rank's local expert e   (i32 [W*E_local], device memory)
 *   smoe_a2a_tokens : all-to-all-v of d-element rows; `send` holds the rows for rank 0, 1, ... (send_rows[w] each: the
 *                     expert-sorted send buffer has that order), `recv` receives recv_rows[w] rows from rank w, rank-major
 *                     (the [source rank][local expert] layout smoe_grouped_gemm takes through group_expert);
 *                     send_rows / recv_rows are HOST i64 [W]
 * wait = SMOE_A2A_INLINE posts the exchange on the caller's `stream` itself (no communication stream, no events, no ticket):
 * in stream order with the kernels either side of it, for a caller that has nothing to run beside the exchange.             */
#define SMOE_A2A_INLINE 2
typedef struct smoe_ctx smoe_ctx;
int smoe_unique_id_bytes(void);
int smoe_unique_id(void* out_id);
int smoe_ctx_create(const void* unique_id, int world_size, int rank, smoe_ctx** out);   /* on the current device */
int smoe_ctx_destroy(smoe_ctx* ctx);
void* smoe_ctx_comm_stream(smoe_ctx* ctx);
int smoe_ctx_world_size(smoe_ctx* ctx);
int smoe_ctx_rank(smoe_ctx* ctx);
int smoe_a2a_counts(smoe_ctx* ctx, const int32_t* send_counts, int32_t* recv_counts, int E_local, void* stream, int wait);
int smoe_a2a_tokens(smoe_ctx* ctx, const void* send, const int64_t* send_rows, void* recv, const int64_t* recv_rows, int d,
                    int dtype, void* stream, int wait);
int smoe_a2a_wait(smoe_ctx* ctx, void* stream);
int64_t smoe_a2a_last_ticket(smoe_ctx* ctx);
int smoe_a2a_wait_ticket(smoe_ctx* ctx, int64_t ticket, void* stream);

/* ---- backward of the dense half of the block (training step, engine.py:52-74) -------------------------
 * The linears' backward needs no kernel of its own: dgrad = smoe_grouped_gemm with one row group on the transposed weight
 * image (smoe_transpose_cast), wgrad = smoe_grouped_wgrad_rows with one group, bias gradient = smoe_group_colsum.
 * smoe_layernorm_bwd: backward of nn.LayerNorm(d, eps) (models/vision_transformer.py:303-311) from x alone (statistics
 * recomputed): dx = rstd (g - mean(g) - xhat mean(g xhat)) [+ dres: the gradient arriving over the residual connection that
 * bypasses the norm, fused], g = dy gamma; dgamma_dbeta [2 d] = (sum dy xhat, sum dy), deterministic (partial rows per
 * workgroup in `workspace`, added in order).  x / dx / dres f32 [T, d]; dy f32 / f16 / bf16; d % 4 == 0, d <= 1024.   */
/* smoe_gate_dgrad: the router linear's input gradient dx [T, d] = dl [T, E] W [E, d] (f32 in, out f32 / f16 / bf16): K = E is too
 * thin for the matrix cores, the kernel is bound by its [T, d] store.                                                            */
int smoe_gate_dgrad(const float* dl, const float* w, int64_t T, int E, int d, void* out, int out_dtype, void* stream);
size_t smoe_layernorm_bwd_workspace_bytes(int64_t T, int d);
int smoe_layernorm_bwd(const float* x, const void* dy, int dy_dtype, const float* gamma, const float* dres, float eps, int64_t T,
                       int d, float* dx, float* dgamma_dbeta, void* workspace, size_t workspace_bytes, void* stream);

/* ---- optimizer side of the training step (engine.py:68-74: timm NativeScaler around torch.optim.AdamW; SURVEY.md 8f
 * rank 3).  Everything stays on the device -- loss scale, non-finite flag, clip coefficient, step count -- so a step has
 * no host sync, and a gradient is read twice in all (norm pass, update pass) instead of four times.
 * smoe_grad_sumsq : partial[b] = sum over block b (smoe_grad_sumsq_blocks(n) blocks of 16384 elements) of
 *                   (g * *inv_scale)^2, deterministic; *found_inf = 1 when any scaled-back element is inf / nan
 *                   (GradScaler.unscale_'s check; the caller zeroes found_inf once per step); inv_scale may be NULL (= 1)
 * smoe_adamw_step : torch.optim.AdamW arithmetic on f32 p / m / v with the gradient g (f32 / f16 / bf16) multiplied by
 *                   *grad_mult (NULL = 1: e.g. inv_scale x clip coefficient): p *= 1 - lr wd; m = lerp(m, g, 1 - b1);
 *                   v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps), t = *step
 *                   (device f32, already advanced); the whole update is skipped when *found_inf != 0 (found_inf may be NULL).
 *                   beta1 / beta2 are DOUBLES (ABI 30): 1 - b1, 1 - b2, 1 - b1^t and sqrt(1 - b2^t) are taken in double on the
 *                   device and rounded once -- in f32, 1.0f - 0.999f is off by 1.3e-5 of itself on every element of every update;
 *                   lerp is torch's (g - b1 (g - m) where 1 - b1 >= 0.5, so beta1 = 0 gives m = g exactly)
 * smoe_amp_update : GradScaler.update(): found_inf ? (scale *= backoff, tracker = 0)
 *                                                 : (++tracker == interval ? (scale *= growth, tracker = 0) : -)
 * smoe_step_advance: *step += 1 unless *found_inf != 0                                                                  */
int64_t smoe_grad_sumsq_blocks(int64_t n);
int smoe_grad_sumsq(const void* g, int g_dtype, int64_t n, const float* inv_scale, float* partial, float* found_inf,
                    void* stream);
int smoe_adamw_step(float* p, const void* g, int g_dtype, float* m, float* v, int64_t n, float lr, double beta1, double beta2,
                    float eps, float weight_decay, const float* step, const float* grad_mult, const float* found_inf,
                    void* stream);
/* Multi-tensor forms of the two passes: ONE launch for every gradient / parameter of the step (torch's `foreach` / fused
 * AdamW play this role upstream).  tab = int64 [5][n_tensors] in device memory: rows p, g, exp_avg, exp_avg_sq (addresses) and
 * n (elements); the sumsq form reads rows g and n only.  hyp = f32 [2][n_tensors]: lr, weight_decay.  blk = int32 [2][n_blocks]:
 * the tensor of workgroup b and the 16,384-element block inside it, blocks in tensor order; partial[b] receives block b's sum.
 * Same arithmetic and the same partial sums as the single-tensor forms.  shadow (may be NULL) = int64 [2][n_tensors]: the address of
 * a 16-bit image of parameter t (0 = none) and its dtype code (SMOE_F16 / SMOE_BF16): the step writes the updated parameter there
 * as well, so the MFMA operand copies the next forward reads need no cast pass of their own (autocast re-casts every weight on
 * every forward upstream; engine.py:52-53).  A step skipped by found_inf leaves parameter and image untouched.               */
int smoe_grad_sumsq_multi(const int64_t* tab, int n_tensors, const int32_t* blk, int64_t n_blocks, int g_dtype,
                          const float* inv_scale, float* partial, float* found_inf, void* stream);
int smoe_adamw_step_multi(const int64_t* tab, const float* hyp, int n_tensors, const int32_t* blk, int64_t n_blocks,
                          int g_dtype, double beta1, double beta2, float eps, const float* step, const float* grad_mult,
                          const float* found_inf, const int64_t* shadow, void* stream);
int smoe_amp_update(float* scale, float* growth_tracker, const float* found_inf, float growth_factor, float backoff_factor,
                    int growth_interval, void* stream);
int smoe_step_advance(float* step, const float* found_inf, void* stream);
/* Weight EMA of the model (timm.utils.ModelEma.update, engine.py:77-78: `ema_v.copy_(ema_v * decay + (1. - decay) * model_v)`),
 * every tensor in ONE launch, in place.  tab = int64 [3][n_tensors] in device memory: rows ema, model (addresses of f32 tensors,
 * 16-byte aligned) and n (elements, 0 allowed); blk = int32 [2][n_blocks] as for smoe_adamw_step_multi.  Per element
 * ema = (ema * decay) + (model * one_minus_decay), three separately rounded f32 operations -- bit-equal to torch's line when the
 * caller passes f32(decay) and f32(1 - decay) with the difference taken in double (for 0.99996 that is not 1.0f - f32(decay)).
 * skip (may be NULL): a device f32 flag; non-zero = the launch writes nothing.  No allocation, no synchronisation.          */
int smoe_ema_update_multi(const int64_t* tab, int n_tensors, const int32_t* blk, int64_t n_blocks, float decay,
                          float one_minus_decay, const float* skip, void* stream);
/* LAMB (timm.optim.Lamb 0.4.12 / 0.5; the DeiT-III recipes' --opt lamb, main.py:90-96, 729-731) on the tables of
 * smoe_adamw_step_multi: tab, blk and shadow as there; hyp = f32 [3][n_tensors]: lr, weight_decay and the adapt flag
 * (weight_decay != 0 or always_adapt; 0 = the tensor's trust ratio is 1).  Four launches per step, every one of which returns at
 * once when *found_inf != 0 (found_inf may be NULL), none of which allocates or synchronises; every sum has a fixed order.
 * smoe_lamb_clip         : ONE workgroup.  partial = the block partials of smoe_grad_sumsq_multi over every gradient of the step
 *                          (n_partials of them, summed in double): out[1] = G = sqrt(sum) * *mult_num / *mult_den (NULL = 1: the
 *                          partials were taken with *mult_den, the optimizer reads its gradients times *mult_num), out[0] = clip =
 *                          G > max_grad_norm ? G / max_grad_norm : 1; max_grad_norm <= 0 = no clipping (timm's None).
 * smoe_lamb_stage1_multi : g' = g * *grad_mult / *clip (NULL = 1 each); exp_avg = exp_avg * beta1 + beta3 * g'; exp_avg_sq =
 *                          exp_avg_sq * beta2 + (1 - beta2) * g'^2, in place; u = (exp_avg / bc1) / (sqrt(exp_avg_sq) / sqrt(bc2) +
 *                          eps) + weight_decay * p with bc1 = 1 - beta1^t, bc2 = 1 - beta2^t (t = *step, already advanced; both 1
 *                          when bias_correction == 0).  u is NOT stored: norms = f32 [2][n_blocks] receives per block sum(p^2) and
 *                          sum(u^2), for tensors with the adapt flag on.
 * smoe_lamb_trust_multi  : one wave per tensor.  first = int32 [n_tensors + 1]: the first block of every tensor (first[n_tensors] =
 *                          n_blocks).  trust[t] = ||p|| / ||u|| from the block partials, in double, 1 where either norm is 0 or the
 *                          adapt flag is off; trust_clip != 0: at most 1.
 * smoe_lamb_stage2_multi : u again, by the same device function from the same operands (the new moments, the old p), then
 *                          p -= lr * (trust[t] * u); where shadow holds an image of p, the updated value is written there too.  */
int smoe_lamb_clip(const float* partial, int64_t n_partials, const float* mult_num, const float* mult_den, float max_grad_norm,
                   const float* found_inf, float* out, void* stream);
int smoe_lamb_stage1_multi(const int64_t* tab, const float* hyp, int n_tensors, const int32_t* blk, int64_t n_blocks, int g_dtype,
                           double beta1, double beta2, float beta3, float eps, int bias_correction, const float* step,
                           const float* grad_mult, const float* clip, const float* found_inf, float* norms, void* stream);
int smoe_lamb_trust_multi(const float* norms, int64_t n_blocks, const int32_t* first, const float* hyp, int n_tensors,
                          int trust_clip, const float* found_inf, float* trust, void* stream);
int smoe_lamb_stage2_multi(const int64_t* tab, const float* hyp, int n_tensors, const int32_t* blk, int64_t n_blocks, double beta1,
                           double beta2, float eps, int bias_correction, const float* step, const float* trust,
                           const float* found_inf, const int64_t* shadow, void* stream);

/* ---- the recipe around the model (engine.py:46-47, 54; main.py:505-517 timm.data.Mixup, main.py:653-661 timm.loss.
 * SoftTargetCrossEntropy / LabelSmoothingCrossEntropy; the reference's default run is --mixup 0.8 --cutmix 1.0 --smoothing 0.1).
 * smoe_mixup_images : Mixup / CutMix IN PLACE on x f32 [B, C, H, W] (contiguous, B even, C*H*W < 2^31).  Sample b is paired with
 *                     j = B-1-b.  Per sample: lam[b], one_minus[b] (f32, rounded by the caller) and box[b] = (yl, yh, xl, xh) i32.
 *                     An empty box (yh <= yl or xh <= xl) = Mixup: out_b = (x_b * lam[b]) + (x_j * one_minus[b]), three separately
 *                     rounded f32 operations, bit-equal to torch's `x.mul_(lam).add_(x.flip(0).mul_(1 - lam))`.  A non-empty box =
 *                     CutMix: out_b = x_j inside the box, x_b outside.  lam[b] == 1: the sample is left untouched (nothing of its
 *                     partner leaks in, not even 0 * inf).  Both samples of a pair are computed from the two ORIGINALS, so any mix
 *                     of kinds, factors and boxes inside a pair is right in place (timm's batch, pair and elem modes).  One read and
 *                     one write per element; a pair without a Mixup sample touches only the positions inside its boxes.  16-byte
 *                     accesses when C*H*W % 4 == 0 and x is 16-byte aligned, element-wise otherwise.
 * smoe_mixup_target : out f32 [B, num_classes] = (y1 * lam[b]) + (y2 * one_minus[b]), y1 = one_hot(labels[b]), y2 =
 *                     one_hot(labels[B-1-b]) with values on / off (timm's mixup_target: off = smoothing / num_classes, on = 1 -
 *                     smoothing + off), same three roundings.  labels i64 [B].  A label outside [0, num_classes) contributes `off`
 *                     everywhere (no class is "on"); nothing is read back to check it.  One launch.
 * smoe_soft_ce_fwd  : logits [B, C] (f32 / f16 / bf16, computed in f32) with the target of a row in ONE of two forms -- target f32
 *                     [B, C] (labels NULL): row loss = sum(-t log_softmax(x)) = lse sum(t) - dot(t, x); or labels i64 [B] (target
 *                     NULL) + smoothing: t = smoothing / C + (1 - smoothing) [c == label], sum(t) = 1 (smoothing 0 = cross-entropy;
 *                     a label outside [0, C) puts the (1 - smoothing) nowhere).  Writes f32 [B] each: row_loss, row_max, row_logsum
 *                     (lse = max + log(sum of exp(x - max)), kept as its two terms) and row_tsum, and *loss = mean of row_loss, summed
 *                     in a fixed order: the same bits run to run.  Each logit and target is read once (online max / sum).  Two
 *                     launches.  row_logsum is NaN whenever the log-sum-exp is not finite (a +inf or NaN logit, a row of -inf): that
 *                     row's loss and whole gradient are then NaN, as torch's log_softmax makes them.
 * smoe_soft_ce_bwd  : dlogits [B, C] (the logits' dtype, rounded once from f32) = *g (exp(x - max - logsum) sum(t) - t) / B; g is a DEVICE f32
 *                     scalar (the gradient of the mean loss: it carries the loss scale).  Rows are independent.  B <= 65535.  One launch.
 *                     Which non-finite value appears (inf or NaN) is not preserved: a -inf logit under a positive target gives a
 *                     NaN row loss where exact arithmetic gives +inf.
 * C <= 2^30.  B == 0 returns 0 at once; no allocation, no synchronisation, no atomics: all four can be captured.                             */
int smoe_mixup_images(float* x, int64_t B, int C, int H, int W, const float* lam, const float* one_minus, const int32_t* box,
                      void* stream);
int smoe_mixup_target(const int64_t* labels, const float* lam, const float* one_minus, float on, float off, int64_t B,
                      int num_classes, float* out, void* stream);
int smoe_soft_ce_fwd(const void* logits, int dtype, const float* target, const int64_t* labels, float smoothing, int64_t B, int C,
                     float* row_loss, float* row_max, float* row_logsum, float* row_tsum, float* loss, void* stream);
int smoe_soft_ce_bwd(const void* logits, int dtype, const float* target, const int64_t* labels, float smoothing, int64_t B, int C,
                     const float* row_max, const float* row_logsum, const float* row_tsum, const float* g, void* dlogits, void* stream);

/* ---- evaluation metrics (engine.py:99-113: `loss = criterion(output, target)`, `acc1, acc5 = accuracy(output, target, topk=(1, 5))`
 * and three `.item()` reads per batch; timm.utils.accuracy) ------------------------------------------------------------------------------
 * smoe_eval_metrics : logits [B, C] (f32 / f16 / bf16, computed in f32), labels i64 [B]; ks = a HOST array of nk values (1 <= nk <= 4,
 *                     every k >= 1; read before the call returns).  Two launches, each logit read once.
 *   row_loss f32 [B]  : the row's cross-entropy -- smoe_soft_ce_fwd's label form at smoothing 0, the same arithmetic in the same order:
 *                       bit-equal to its row_loss for a label inside [0, C).
 *   row_rank i32 [B]  : the number of classes that come before the label's class in a stable descending order of the row,
 *                       #{c : x_c > x_t} + #{c < label : x_c == x_t} with x_t = logits[b, label], where a NaN is the largest value and
 *                       two NaNs are equal (torch.topk's order); ties go to the LOWER index.  The label is in the top k iff row_rank < k.
 *                       On a row without a logit equal to x_t this is what `output.topk(k, 1, True, True)` + `eq` decide; on a tie
 *                       torch.topk's pick is unspecified and this rule is the contract.
 *   batch f32 [1+nk]  : batch[0] = mean of row_loss, summed in smoe_soft_ce_fwd's fixed order (bit-equal to its *loss);
 *                       batch[1 + i] = (count_i * 100) * f32(1 / B) in f32 with count_i = #{rows : row_rank < ks[i]} -- the bits of timm's
 *                       `correct[:k].reshape(-1).float().sum(0) * 100.0 / B` as torch computes it on the device (a division by a host
 *                       scalar is a multiplication by its f32 reciprocal there; up to one ulp from the true quotient).
 *   acc f64 [2+nk]    : may be NULL.  acc[0] += sum of (double)row_loss[b] in a fixed order, acc[1] += B, acc[2 + i] += count_i: a
 *                       plain read-add-write by one thread, ordered by the stream, NO atomics -- the epoch's meter without a host read
 *                       per batch.  One accumulator used from two streams at once is the caller's error.
 * Non-finite inputs and bad labels: a label outside [0, C) gives row_rank = INT32_MAX (never correct) and row_loss = NaN, and nothing
 * is read out of bounds (where torch device-asserts).  A NaN or +inf logit, or a row of -inf, makes that row's loss NaN as in
 * smoe_soft_ce_fwd; its rank still follows the rule above.  Other rows are untouched; batch[0] and acc[0] take the poison through the
 * sum, the counts stay exact.
 * 0 < C <= 2^30, B < 2^31.  16-byte accesses when C % 8 == 0 and logits is 16-byte aligned, element-wise otherwise.  B == 0 returns 0
 * at once; arguments are checked before any launch; no allocation, no synchronisation: it can be captured.                            */
int smoe_eval_metrics(const void* logits, int dtype, const int64_t* labels, int64_t B, int C, const int* ks, int nk,
                      float* row_loss, int32_t* row_rank, float* batch, double* acc, void* stream);

/* ---- knowledge distillation (main.py:688 `criterion = DistillationLoss(...)`; losses.py:53-72) -------------------------------------
 * The distillation term between the student's distillation logits and a teacher's logits, both [B, C], each f32 / f16 / bf16 with its
 * own dtype code, and its blend with the base loss.  mode 0 = soft, 1 = hard; tau > 0 (soft only); alpha.
 * smoe_distill_fwd : soft: s = student / tau, t = teacher / tau; row_val[b] = sum_c p_t (log p_t - log p_s), p = softmax -- what
 *                    F.kl_div(log_softmax(s), log_softmax(t), reduction='none', log_target=True).sum(1) gives; *distill_loss =
 *                    (sum of row_val) * tau^2 / (B * C).  hard: row_val[b] = logsumexp(student[b]) - student[b, argmax_c teacher[b]]
 *                    (F.cross_entropy against the teacher's argmax), *distill_loss = mean of row_val.  The argmax is torch.argmax's:
 *                    the first maximal index, and a NaN counts as the maximum (the first NaN wins).
 *                    *loss = *base_loss * (1 - alpha) + *distill_loss * alpha; base_loss is a DEVICE f32 scalar.
 *                    row_val is f64 [B].  Also written, for the backward: row_stats f64 [4, B] = the student's row maximum (of the raw
 *                    logits) and log of the sum of exp((x - max) / tau), the teacher's (soft; zeros in hard mode), and row_label i32 [B] =
 *                    the argmax (hard; -1 in soft mode).  Both logit rows are read once (online max / sum; the soft term rides on the
 *                    teacher's running maximum); the rows are summed in a fixed order: the same bits run to run.  Two launches.
 *                    The arithmetic is double precision throughout (the soft term cancels when the student is close to the teacher):
 *                    the two scalars and dlogits carry the f64 result's error (far below an f32 ulp) plus one rounding.
 * smoe_distill_bwd : dlogits [B, C] in the student's dtype (rounded once from f32) = *g * alpha * tau / (B * C) * (p_s - p_t) (soft) or
 *                    *g * alpha / B * (p_s - onehot(row_label)) (hard); g is a DEVICE f32 scalar (the gradient of the blended loss: it
 *                    carries the loss scale).  The teacher gets no gradient; the base loss' gradient is *g * (1 - alpha), the caller's.
 *                    B <= 65535.  One launch.
 * Non-finite inputs: nothing is masked.  A NaN or +inf logit in either row, or a row of -inf, makes that row's value and (through a NaN
 * log-sum) its whole gradient NaN; a -inf TEACHER logit makes the soft row value NaN (0 * -inf, as the reference's
 * exp(log p_t) * (log p_t - log p_s) does); a -inf STUDENT logit under a finite teacher makes it +inf.  Other rows are untouched; the
 * two scalars take the poison through the sum.  Which non-finite value appears (inf or NaN) is not preserved.
 * 0 < C <= 2^30, B < 2^31 (forward).  16-byte accesses when C % 8 == 0 and student, teacher and dlogits are 16-byte aligned,
 * element-wise otherwise.  B == 0 returns 0 at once; no allocation, no synchronisation, no atomics: both can be captured.          */
int smoe_distill_fwd(const void* student, int s_dtype, const void* teacher, int t_dtype, int mode, float tau, float alpha,
                     const float* base_loss, int64_t B, int C, double* row_val, double* row_stats, int32_t* row_label,
                     float* distill_loss, float* loss, void* stream);
int smoe_distill_bwd(const void* student, int s_dtype, const void* teacher, int t_dtype, int mode, float tau, float alpha, int64_t B,
                     int C, const double* row_stats, const int32_t* row_label, const float* g, void* dlogits, void* stream);

/* ---- binary cross-entropy with logits (main.py:663-664 `criterion = torch.nn.BCEWithLogitsLoss()` under --bce-loss; engine.py:49-50
 * `targets = targets.gt(0.0).type(targets.dtype)`) ------------------------------------------------------------------------------------
 * logits [B, C] (f32 / f16 / bf16, computed in f32), target f32 [B, C].  binarize != 0: every target is read as t' = (t > 0 ? 1 : 0) --
 * engine.py:50's strict `> 0`: -0.0, 0.0, a negative value and NaN give 0; binarize == 0: t' = t.
 * smoe_bce_fwd : element loss = max(x, 0) - x t' + log1p(exp(-|x|)) (torch's stable form), in f32.  row_loss f32 [B] = the row's sum:
 *                one workgroup per row, the f32 elements added in double on a fixed tree and rounded once.  *loss = (sum of row_loss in
 *                a fixed order, in double) * 1 / (B C), rounded once to f32: reduction='mean', the only one the reference constructs.
 *                The same bits run to run; a row's loss does not depend on the other rows.  Two launches.
 * smoe_bce_bwd : dlogits [B, C] (the logits' dtype, rounded once from f32) = *g (sigmoid(x) - t') / (B C); g is a DEVICE f32 scalar
 *                (the gradient of the mean loss: it carries the loss scale).  sigmoid(x) - t' is formed from e = exp(-|x|) as
 *                (1 - t') - e / (1 + e) for x >= 0 and e / (1 + e) - t' for x < 0: nothing overflows, and 1 - sigmoid keeps its
 *                precision for large x.  Purely element-wise.  One launch.
 * Non-finite inputs: an element whose logit is NaN or infinite, or whose (unbinarized) target is, gives a non-finite row_loss for its
 * row and a non-finite *loss; which of inf / NaN appears is not preserved (torch's own formula gives NaN for x = +inf, t = 1).
 * dlogits[b, c] depends on logits[b, c], target[b, c] and *g only: a NaN or infinite logit makes its own gradient element NaN and
 * touches no other; other rows' row_loss keep their bits.
 * B <= 65535 (one workgroup per row / grid row), 0 < C <= 2^30.  16-byte accesses when C % 8 == 0 and logits, target (and dlogits) are
 * 16-byte aligned, element-wise otherwise.  B == 0 returns 0 at once; all arguments (null pointers, dtype code, sizes, alignment of
 * the f32 buffers) are checked before any launch; no allocation, no synchronisation, no atomics: both can be captured.             */
int smoe_bce_fwd(const void* logits, int dtype, const float* target, int binarize, int64_t B, int C, float* row_loss, float* loss,
                 void* stream);
int smoe_bce_bwd(const void* logits, int dtype, const float* target, int binarize, int64_t B, int C, const float* g, void* dlogits,
                 void* stream);

/* ---- SwitchableLayerNorm (models/layers.py:31-157, the rule of its forward at 105-151; the `router` of SwitchableVisionTransformer,
 * models/vision_transformer.py:407 and 591) ---------------------------------------------------------------------------------------------
 * x [T, d] f32; weights, biases, centroids [K, d] f32.  Per row: mean and biased variance over d, xhat = (x - mean) rsqrt(var + eps);
 * the row's bucket b; y = xhat weights[b] + biases[b] (weights == NULL: y = xhat, biases must be NULL too; biases == NULL: no shift).
 * The bucket is buckets_in[t] (int64 [T]) when that is given, else bucket_all (>= 0) for every row, else -- both unused, bucket_all ==
 * -1 -- the SELECTED one: argmin_k sum_j (x_j - c_kj)^2 over the raw row, the first minimum, a NaN distance counting as the smallest
 * and the first NaN winning (torch.argmin).  The distances are accumulated in double in this direct form, so the selection is the
 * float64 evaluation's wherever the two smallest distances differ by more than float64's own error (upstream's f32 torch.cdist takes
 * the expanded form and misassigns rows near a bisector).  K == 1 selects bucket 0 and never reads centroids (may be NULL); centroids
 * are not read either when the buckets are given.
 * smoe_switch_ln_supported : d % 4 == 0, 4 <= d <= 1024, 1 <= K <= 32.
 * smoe_switch_ln_fwd : y f32 [T, d], buckets_out int64 [T] (the bucket used, also when it was given).  One launch, one wave per row,
 *                    two-pass statistics in registers; x is not written.  No row statistics are kept: the backward recomputes them
 *                    from x, as smoe_layernorm_bwd does.  A given bucket outside [0, K) reads nothing from the tables: its y row is NaN
 *                    and buckets_out repeats the value.
 * smoe_switch_ln_bwd : dy [T, d] f32 / f16 / bf16; dx f32 [T, d] = rstd (g - mean(g) - xhat mean(g xhat)), g = dy weights[b] (nothing
 *                    flows through the selection; a bucket outside [0, K): a NaN row); dweights[k] = sum over the rows of bucket k of
 *                    dy xhat, dbiases[k] = sum of dy, both f32 [K, d] (both NULL: not computed).  The sums are deterministic: partial
 *                    tables per workgroup in the workspace, added in a fixed order -- the same bits run to run -- and the rows of an
 *                    empty bucket are exact zeros.  centroids get no gradient.  Four launches (dx; column sums; two reduce stages).
 * Non-finite inputs: nothing is masked.  A NaN in a row of x makes that row's y (and dx) NaN and every distance NaN, so the row selects
 * bucket 0; no other row changes a bit.  A NaN centroid k draws every finite row to k (the smallest such k).  A NaN row of dy poisons
 * its own dx row and the two gradient rows of its own bucket, nothing else.
 * T >= 0 (T == 0: the forward returns at once; the backward writes zero gradients); rows are addressed in 64 bits.  x, y, dx and the
 * tables 16-byte aligned.  Arguments are checked before any launch; no allocation, no host read, no atomics: both can be captured.  */
int smoe_switch_ln_supported(int d, int K);
int smoe_switch_ln_fwd(const float* x, const float* weights, const float* biases, const float* centroids, const int64_t* buckets_in,
                       int bucket_all, float eps, int64_t T, int d, int K, float* y, int64_t* buckets_out, void* stream);
size_t smoe_switch_ln_bwd_workspace_bytes(int64_t T, int d, int K);
int smoe_switch_ln_bwd(const float* x, const void* dy, int dy_dtype, const float* weights, const int64_t* buckets, float eps,
                       int64_t T, int d, int K, float* dx, float* dweights, float* dbiases, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- counter-based dropout (main.py --drop: pos_drop, proj_drop, the experts' Dropout behind GELU) --------------------------------
 * The mask is a pure function of (key, first_block, element index): nothing is stored for the backward, which calls smoe_dropout on
 * the gradient with the forward's key (dx = dropout_same_key(dy)), and the host can reproduce every mask bit (tests/_dropout_cases.py).
 * THE RULE: Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85.  key: DEVICE int64 [2] =
 * (k, c), read from memory as uint64 by every launch (never by value: a replayed graph sees the key its replay drew).  Elements are
 * numbered row-major over the logical [rows, cols] tensor; element e lies in block b = first_block + e / 8 (first_block: 0, or the
 * number of 8-element blocks in front of this piece of a larger tensor).  Block b: Philox key (lo32 k, hi32 k), counter (lo32 b, hi32
 * b, lo32 c, hi32 c) -> r0..r3; element 8 b + 2 j + h (j 0..3, h 0..1) draws u = (r_j >> 16 h) & 0xffff and is KEPT iff u < thr16.
 * thr16 = round((1 - p) * 65536) in [0, 65536]; scale = (float)(65536.0 / thr16) formed in double on the host (0 for thr16 == 0): the
 * inverse of the keep probability really applied.  f32 arithmetic, one rounding per operation: t = f32(x) * scale; with row_scale
 * (f32 [rows]) t = t * row_scale[row]; a dropped element is SELECTED to +0.0 (a dropped NaN / inf gives 0, a kept one propagates);
 * smoe_dropout_add then forms residual + t; one round-to-nearest-even into the output dtype.  The mask does not depend on the grid,
 * the dtypes, or on which of the two entry points runs.
 * smoe_dropout     : y [rows, cols] (dtype_out) from x (dtype_in), any pairing of f32 / f16 / bf16; y may be x when the dtypes are equal.
 * smoe_dropout_add : out f32 = residual f32 + t(h); h f32 / f16 / bf16; out may be residual (never h).
 * cols % 8 == 0, cols > 0; rows >= 0 (0 returns at once); rows * cols * 4 must fit in int64; x, y, h, residual, out 16-byte aligned, key
 * 8-byte aligned.  Null pointers, sizes, thr16 > 65536, dtype codes and alignment are refused with a message before any launch.  One
 * launch of 256-thread workgroups (at most 4096, a grid stride behind that), 8 elements per lane and trip; no LDS, no atomics, no
 * allocation, no host read: both can be captured.                                                                                 */
int smoe_dropout(const void* x, void* y, const float* row_scale, const int64_t* key, uint64_t first_block, int64_t rows, int64_t cols,
                 uint32_t thr16, float scale, int dtype_in, int dtype_out, void* stream);
int smoe_dropout_add(const void* h, const float* residual, const float* row_scale, float* out, const int64_t* key,
                     uint64_t first_block, int64_t rows, int64_t cols, uint32_t thr16, float scale, int dtype_h, void* stream);

/* ---- small helpers ------------------------------------------------------------------------------------
 * elementwise cast between dtypes (weight shadow copies; not on the per-step path)                  */
int smoe_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SLIMMOE_H */
