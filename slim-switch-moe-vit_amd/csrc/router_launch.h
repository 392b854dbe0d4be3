// Host side of the router launches (router.hip, router16.hip, gate.hip): what an entry point knows travels in ONE struct, the
// pass sequence is written ONCE.  No device code here: the kernels keep their positional scalar parameters.
#pragma once
#include "router16_kernel.h"  // SkipGateArgs / HistArgs: the two plain structs the 16-lane kernels take by value

// Everything one of the three extern "C" entry points (smoe_router_topk, smoe_ln_router_topk, smoe_gate_ln_router) was handed,
// filled once there and passed down by const reference.
struct RouterArgs {
  const char* entry;  // the entry point's name, for error text
  const void* x;
  int x_dtype;
  // LayerNorm in front of the router (ln_on = false: the router reads x as it is, none of the six is looked at)
  bool ln_on;
  const float* ln_g;
  const float* ln_b;
  float ln_eps;
  void* xn16;
  int xn16_dtype;
  float* xn32;
  const float* wg;
  const float* bg;
  const float* noise;
  int64_t T;
  int d, E, k, gate_kind;  // gate_kind without its flag bits
  int64_t* idx;
  float* score;
  float* logits;
  float* probs;
  r16::SkipGateArgs gate;  // token-skip gate (smoe_gate_ln_router only; all NULL otherwise)
  int32_t* hist;           // chunk histogram for the dispatch plan, or NULL
  int32_t* redo_count;     // workspace: [16 B: redo counter, redo-pass ticket, pad][T x i32 redo list]
  int32_t* redo_list;
  bool all_f64;       // SMOE_ROUTER_ALL_F64: every token through the f64 pass
  bool ws_kept_zero;  // SMOE_ROUTER_WS_KEPT_ZERO: the counter words are zero on entry, no clearing launch
  hipStream_t stream;
};

// The two flag bits of the router entry points' gate_kind argument, decoded here and nowhere else.
inline void router_decode_gate_kind(RouterArgs& a, int gate_kind) {
  a.all_f64 = (gate_kind & SMOE_ROUTER_ALL_F64) != 0;
  a.ws_kept_zero = (gate_kind & SMOE_ROUTER_WS_KEPT_ZERO) != 0;
  a.gate_kind = gate_kind & 0xff;
}

// Checks and carves the workspace; smoe_router_workspace_bytes is the only size rule.
inline int router_take_workspace(RouterArgs& a, void* workspace, size_t workspace_bytes) {
  SMOE_REQUIRE(workspace && workspace_bytes >= smoe_router_workspace_bytes(a.T), "%s: workspace too small", a.entry);
  a.redo_count = reinterpret_cast<int32_t*>(workspace);
  a.redo_list = reinterpret_cast<int32_t*>((char*)workspace + 16);
  return 0;
}

// f(XT{}) with the element type of a.x
template <typename F> int router_by_x_dtype(const RouterArgs& a, F&& f) {
  switch (a.x_dtype) {
    case SMOE_F32: return f(float{});
    case SMOE_F16: return f(f16{});
    case SMOE_BF16: return f(bf16_bits{});
  }
  smoe_set_error("%s: bad x_dtype %d", a.entry, a.x_dtype);
  return 1;
}

// The numbers in which the four launchers' pass sequences differ.
struct RouterPlan {
  int grid_f32;          // f32 pass
  int grid_f64;          // f64 pass over all tokens; the redo pass runs min(grid_f64, redo_cap) workgroups
  int redo_cap;          // the redo list is short (~1e-4 T): surplus waves exit at once
  bool f32_writes_rows;  // the f32 pass stores rows an all-f64 run still needs (= LayerNorm on)
  const char* name_f32;  // SMOE_CHECK_LAUNCH names
  const char* name_f64;
  const char* name_redo;
};

// The pass sequence.  launch_f32 / launch_f64 are callables (grid, redo_count, redo_list) that hold one launch each; the f64
// pass walks the redo list, or all tokens when handed none.
template <typename F32, typename F64>
int run_router_passes(const RouterArgs& a, const RouterPlan& p, F32&& launch_f32, F64&& launch_f64) {
  if (a.all_f64 && !p.f32_writes_rows) {
    launch_f64(p.grid_f64, nullptr, nullptr);
    SMOE_CHECK_LAUNCH(p.name_f64);
    return 0;
  }
  if (!a.ws_kept_zero) {  // (a kept workspace is zero already: the redo pass clears its counter words on the way out)
    hipError_t me = smoe_zero_words(a.redo_count, 4, a.stream);
    if (me != hipSuccess) {
      smoe_set_error("%s: counter clear failed: %s", a.entry, hipGetErrorString(me));
      return (int)me;
    }
  }
  launch_f32(p.grid_f32, a.redo_count, a.redo_list);
  SMOE_CHECK_LAUNCH(p.name_f32);
  if (a.all_f64) {  // the f32 pass ran for its stores; nothing walks its list (the caller's workspace is not a kept one)
    launch_f64(p.grid_f64, nullptr, nullptr);
    SMOE_CHECK_LAUNCH(p.name_f64);
    return 0;
  }
  launch_f64(p.grid_f64 < p.redo_cap ? p.grid_f64 : p.redo_cap, a.redo_count, a.redo_list);
  SMOE_CHECK_LAUNCH(p.name_redo);
  return 0;
}

int smoe_router16_try(const RouterArgs& a);  // router16.hip: -1 when the shape is not covered by the 16-lane / matrix-core kernels
