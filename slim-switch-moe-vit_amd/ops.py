"""Python face of the C-ABI (include/slimmoe.h): torch tensors in, torch tensors out.

Torch is plumbing here (device memory, streams); every function below launches hand-written HIP
kernels from libslimmoe_hip.so on torch's current stream and raises if that library is missing.
Shapes / dtypes / contiguity are validated here, before the C call (SURVEY.md 8b error convention).
"""
from __future__ import annotations

import ctypes
import functools
from typing import Optional

import torch

from . import _lib
from ._cache import StreamCache

F32, F16, BF16 = 0, 1, 2
GATE_NAIVE, GATE_SWITCH = 0, 1
EPI_NONE, EPI_GELU, EPI_GELU_GRAD = 0, 1, 2

_DT = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
# grouped GEMM variant the modules use: 9 = the persistent kernel (one workgroup per CU walking tiles; auto tile height and
# schedule), bit-identical to 4 = one workgroup per tile (kept for A/B: SLIMMOE_GEMM_VARIANT=4)
import os as _os
DEFAULT_GEMM_VARIANT = int(_os.environ.get("SLIMMOE_GEMM_VARIANT", "9"))


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _DT[dt]
    except KeyError:
        raise TypeError(f"unsupported dtype {dt}; expected float32/float16/bfloat16") from None


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # the current stream's handle without building a Stream object


def _stream(t: torch.Tensor):
    """The HIP stream torch would launch on for ``t``'s device right now (every launch function takes it).  ~250 calls per forward:
    torch.cuda.current_stream() costs ~4.5 us each (a Python Stream object per call), the raw getter a tenth of that."""
    idx = t.device.index
    _lib.init_device(idx)  # first touch of a device: all launch attributes set before any launch
    if _raw_stream is not None:
        return _raw_stream(idx)
    return torch.cuda.current_stream(t.device).cuda_stream


# ---- optional per-launch timing (bench.py's roofline leg): HIP events on the stream the kernels run on ----
_PROFILE = None  # list of (name, meta, start_event, end_event) while enabled


_PROFILE_ONLY = None  # optional set of launch names to time (None = all)


def profile_begin(only=None):
    """Start recording per-launch HIP events.  ``only``: restrict to these launch names (each timed launch costs the
    host two event records -- with the expert-parallel pipeline the host has no slack for timing every launch)."""
    global _PROFILE, _PROFILE_ONLY
    _PROFILE = []
    _PROFILE_ONLY = set(only) if only is not None else None


def profile_end():
    """-> list of (name, meta, milliseconds); call after a device synchronize."""
    global _PROFILE
    rec, _PROFILE = _PROFILE or [], None
    return [(n, m, s.elapsed_time(e)) for n, m, s, e in rec]


class _timed:
    def __init__(self, name, meta, ref):
        self.on = _PROFILE is not None and (_PROFILE_ONLY is None or name in _PROFILE_ONLY)
        if self.on:
            self.name, self.meta, self.ref = name, meta, ref

    def __enter__(self):
        if self.on:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record(torch.cuda.current_stream(self.ref.device))

    def __exit__(self, *a):
        if self.on:
            self.e.record(torch.cuda.current_stream(self.ref.device))
            _PROFILE.append((self.name, self.meta, self.s, self.e))


def _chk(t: torch.Tensor, name: str, dtype=None, ndim=None, align: int = 16):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: must live on the GPU (got {t.device}); the MoE hot path has no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError(f"{name}: expected {ndim} dims, got {tuple(t.shape)}")
    if t.data_ptr() % align != 0 and t.numel() > 0:
        raise RuntimeError(f"{name}: data pointer must be {align}-byte aligned")


_router_ws = {}   # (device index, stream) -> uint8 workspace whose counter words are zero between calls
# gate_kind flags of smoe_router_topk / smoe_ln_router_topk (include/slimmoe.h: SMOE_ROUTER_ALL_F64, SMOE_ROUTER_WS_KEPT_ZERO)
ALL_F64 = 0x100        # every token through the f64 pass (test mode)
WS_KEPT_ZERO = 0x200   # "the workspace's counter words are zero": no clearing launch
GATE_WITH_LN, GATE_WS_KEPT_ZERO = 1, 2   # the bits of smoe_gate_ln_router's with_ln


def _router_call_workspace(dev: torch.device, T: int, all_f64: bool = False):
    """(workspace, its size in bytes, gate_kind flag bits) for one call of a router entry point."""
    ws_bytes = _lib.load().smoe_router_workspace_bytes(T)
    if all_f64:
        # (the all-f64 test mode runs its f32 pass without a redo pass behind it: it gets a scratch workspace and the clearing launch)
        return torch.empty(ws_bytes, dtype=torch.uint8, device=dev), ws_bytes, ALL_F64
    return _router_workspace(dev, ws_bytes), ws_bytes, WS_KEPT_ZERO


def _router_workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    """The router's redo workspace (counter words + token list), one per device and stream, allocated ZEROED once: every
    redo pass clears the counter words on its way out (csrc/router16_kernel.h), so no call has to launch a clearing kernel
    in front of the router -- the caller says so with WS_KEPT_ZERO.  Keyed by the stream: two compute streams never share
    counters; a captured graph replays on the tensor it captured."""
    key = (dev.index, _raw_stream(dev.index) if _raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream)
    t = _router_ws.get(key)
    if t is None or t.numel() < nbytes:
        t = _router_ws[key] = torch.zeros(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
    return t


def router_topk(x: torch.Tensor, wg: torch.Tensor, bg: Optional[torch.Tensor], k: int, gate_kind: int = GATE_NAIVE,
                noise: Optional[torch.Tensor] = None, want_logits: bool = False, want_probs: bool = False,
                force_f64: bool = False):
    """(idx int64 [T,k], score f32 [T,k], logits f32 [T,E] | None, probs f32 [T,E] | None)."""
    _chk(x, "x", ndim=2)
    _chk(wg, "wg", torch.float32, 2)
    T, d = x.shape
    E = wg.shape[0]
    if wg.shape[1] != d:
        raise RuntimeError(f"wg: expected [E,{d}], got {tuple(wg.shape)}")
    if bg is not None:
        _chk(bg, "bg", torch.float32, 1)
        if bg.shape[0] != E:
            raise RuntimeError("bg: expected [E]")
    if noise is not None:
        _chk(noise, "noise", torch.float32, 2)
        if tuple(noise.shape) != (T, E):
            raise RuntimeError("noise: expected [T,E]")
    idx = torch.empty((T, k), dtype=torch.int64, device=x.device)
    score = torch.empty((T, k), dtype=torch.float32, device=x.device)
    logits = torch.empty((T, E), dtype=torch.float32, device=x.device) if want_logits else None
    probs = torch.empty((T, E), dtype=torch.float32, device=x.device) if want_probs else None
    lib = _lib.load()
    ws, ws_bytes, flags = _router_call_workspace(x.device, T, force_f64)
    with _timed("router", {"bytes": T * d * x.element_size()}, x):
        rc = lib.smoe_router_topk(_ptr(x), dtype_code(x.dtype), _ptr(wg), _ptr(bg), _ptr(noise), T, d, E, k,
                                  gate_kind | flags, _ptr(idx), _ptr(score), _ptr(logits),
                                  _ptr(probs), _ptr(ws), ws_bytes, _stream(x))
    _lib.check(rc, "smoe_router_topk")
    return idx, score, logits, probs


LN_DIMS = (192, 384, 768, 1024)


def layernorm(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float,
              out_dtype: torch.dtype) -> torch.Tensor:
    """LayerNorm over the last dim (d in LN_DIMS) with the output cast fused."""
    _chk(x, "x")
    d = x.shape[-1]
    T = x.numel() // d
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    with _timed("layernorm", {"bytes": T * d * (x.element_size() + out.element_size())}, x):
        rc = _lib.load().smoe_layernorm(_ptr(x), dtype_code(x.dtype), _ptr(weight), _ptr(bias), float(eps), T, d,
                                        _ptr(out), dtype_code(out_dtype), _stream(x))
    _lib.check(rc, "smoe_layernorm")
    return out


def layernorm_bwd(x: torch.Tensor, dy: torch.Tensor, weight: Optional[torch.Tensor], eps: float,
                  dres: Optional[torch.Tensor] = None):
    """Backward of LayerNorm over the last dim from x alone: (dx f32 [same shape] (+ dres), dweight f32 [d], dbias f32 [d])."""
    _chk(x, "x", torch.float32)
    _chk(dy, "dy")
    d = x.shape[-1]
    T = x.numel() // d
    if dy.numel() != x.numel():
        raise RuntimeError("layernorm_bwd: dy must have x's shape")
    if dres is not None:
        _chk(dres, "dres", torch.float32)
    lib = _lib.load()
    dx = torch.empty_like(x)
    gb = torch.empty(2 * d, dtype=torch.float32, device=x.device)
    ws_bytes = lib.smoe_layernorm_bwd_workspace_bytes(T, d)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    with _timed("layernorm_bwd", {"bytes": T * d * (8 + dy.element_size())}, x):
        rc = lib.smoe_layernorm_bwd(_ptr(x), _ptr(dy), dtype_code(dy.dtype), _ptr(weight), _ptr(dres), float(eps), T, d,
                                    _ptr(dx), _ptr(gb), _ptr(ws), ws_bytes, _stream(x))
    _lib.check(rc, "smoe_layernorm_bwd")
    return dx, gb[:d], gb[d:]


def depth_scale_rows(mask: torch.Tensor, keep: float, N: int):
    """(factor f32 [B] = mask / keep, rows f32 [B * N] = the sample's factor on each of its N rows): stochastic depth's division and
    expansion in one launch (smoe_depth_scale_rows)."""
    _chk(mask, "mask", torch.float32, 1, align=4)
    B = mask.shape[0]
    factor = torch.empty(B, dtype=torch.float32, device=mask.device)
    rows = torch.empty(B * int(N), dtype=torch.float32, device=mask.device)
    rc = _lib.load().smoe_depth_scale_rows(_ptr(mask), float(keep), B, int(N), _ptr(factor), _ptr(rows), _stream(mask))
    _lib.check(rc, "smoe_depth_scale_rows")
    return factor, rows


def patchify_cast(images: torch.Tensor, ph: int, pw: int, out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """images f32 [B, C, H, W] -> patch rows [B * gh * gw, C * ph * pw] in 16 bit (smoe_patchify_cast)."""
    _chk(images, "images", torch.float32, 4)
    B, C, H, W = images.shape
    out = torch.empty((B * (H // ph) * (W // pw), C * ph * pw), dtype=out_dtype, device=images.device)
    rc = _lib.load().smoe_patchify_cast(_ptr(images), B, C, H, W, ph, pw, _ptr(out), dtype_code(out_dtype), _stream(images))
    _lib.check(rc, "smoe_patchify_cast")
    return out


def embed_ln(tokens: torch.Tensor, cls_token: torch.Tensor, pos_embed: torch.Tensor, B: int, P: int,
             ln: Optional[tuple] = None, xn_dtype: torch.dtype = torch.float16, dist_token: Optional[torch.Tensor] = None):
    """(x32 [B, P + 1, d], xn | None): the f32 stream cat(cls, tokens) + pos_embed and, with ``ln`` = (weight, bias, eps), its
    LayerNorm in 16 bit from the same pass (smoe_embed_ln).  With ``dist_token`` the stream is cat(cls, dist, tokens) + pos_embed,
    [B, P + 2, d] (smoe_embed_ln2)."""
    _chk(tokens, "tokens", ndim=2)
    d = tokens.shape[1]
    cls = cls_token.detach().reshape(-1)
    pos = pos_embed.detach().reshape(-1, d)
    _chk(cls, "cls_token", torch.float32, 1)
    _chk(pos, "pos_embed", torch.float32, 2)
    npre = 1
    dist = None
    if dist_token is not None:
        dist = dist_token.detach().reshape(-1)
        _chk(dist, "dist_token", torch.float32, 1)
        npre = 2
        if dist.numel() != d or dist.device != tokens.device:
            raise RuntimeError("embed_ln: shapes disagree")
    if cls.numel() != d or pos.shape[0] != P + npre or tokens.shape[0] != B * P:
        raise RuntimeError("embed_ln: shapes disagree")
    x32 = torch.empty((B, P + npre, d), dtype=torch.float32, device=tokens.device)
    xn = torch.empty((B, P + npre, d), dtype=xn_dtype, device=tokens.device) if ln is not None else None
    lg, lb, eps = ln if ln is not None else (None, None, 0.0)
    with _timed("embed_ln", {"bytes": B * (P + npre) * d * (2 + 4 + (2 if ln is not None else 0))}, tokens):
        if dist is None:
            rc = _lib.load().smoe_embed_ln(_ptr(tokens), dtype_code(tokens.dtype), _ptr(cls), _ptr(pos), _ptr(lg), _ptr(lb), float(eps), B, P, d,
                                           _ptr(x32), _ptr(xn), dtype_code(xn_dtype), _stream(tokens))
        else:
            rc = _lib.load().smoe_embed_ln2(_ptr(tokens), dtype_code(tokens.dtype), _ptr(cls), _ptr(dist), _ptr(pos), _ptr(lg), _ptr(lb),
                                            float(eps), B, P, d, _ptr(x32), _ptr(xn), dtype_code(xn_dtype), _stream(tokens))
    _lib.check(rc, "smoe_embed_ln" if dist is None else "smoe_embed_ln2")
    return x32, xn


def layernorm_rows(x: torch.Tensor, row_stride: int, T: int, d: int, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                   eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm of the T rows x.data_ptr() + t * row_stride (f32, d elements each) -> f32 [T, d] (smoe_layernorm_rows); ``out``:
    a contiguous f32 [T, d] to write instead of a new tensor."""
    if not (x.is_cuda and x.dtype == torch.float32):
        raise RuntimeError("layernorm_rows: f32 GPU tensor expected")
    if out is None:
        out = torch.empty((T, d), dtype=torch.float32, device=x.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (T, d) and out.device == x.device):
        raise RuntimeError("layernorm_rows: out must be a contiguous f32 [T, d] on x's device")
    if x.numel() < (T - 1) * int(row_stride) + d:
        raise RuntimeError("layernorm_rows: the last row ends outside x")
    rc = _lib.load().smoe_layernorm_rows(_ptr(x), int(row_stride), _ptr(weight), _ptr(bias), float(eps), T, d, _ptr(out), _stream(x))
    _lib.check(rc, "smoe_layernorm_rows")
    return out


def attention_supported(N: int, head_dim: int) -> bool:
    return bool(_lib.load().smoe_attention_supported(N, head_dim))


def attention(qkv: torch.Tensor, B: int, N: int, H: int, head_dim: int, scale: float, want_lse: bool = False):
    """qkv [B*N, 3*H*head_dim] (or [B,N,3,H,hd]) 16-bit -> softmax(q k^T * scale) v as [B, N, H*head_dim]; with
    ``want_lse`` also the [B, H, N] f32 log2-normalisers the backward needs (returns (out, lse))."""
    _chk(qkv, "qkv")
    if qkv.dtype not in (torch.float16, torch.bfloat16) or qkv.numel() != B * N * 3 * H * head_dim:
        raise RuntimeError("qkv: expected a 16-bit [B,N,3,H,hd] tensor")
    out = torch.empty((B, N, H * head_dim), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device) if want_lse else None
    with _timed("attention", {"flops": 4.0 * B * H * N * N * head_dim}, qkv):
        rc = _lib.load().smoe_attention_fwd(_ptr(qkv), _ptr(out), dtype_code(qkv.dtype), B, N, H, head_dim, float(scale),
                                            _ptr(lse), _stream(qkv))
    _lib.check(rc, "smoe_attention_fwd")
    return (out, lse) if want_lse else out


def attention_bwd_supported(N: int, head_dim: int) -> bool:
    return bool(_lib.load().smoe_attention_bwd_supported(N, head_dim))


def attention_bwd(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, B: int, N: int, H: int,
                  head_dim: int, scale: float) -> torch.Tensor:
    """dqkv (qkv's shape and dtype) of softmax(q k^T scale) v from the forward's ``out`` and ``lse``; N <= 640 (one kernel up to
    N = 256, a dQ and a dK / dV kernel above; no workspace either way)."""
    _chk(qkv, "qkv")
    _chk(out, "out", qkv.dtype)
    _chk(dout, "dout", qkv.dtype)
    _chk(lse, "lse", torch.float32)
    if out.numel() != B * N * H * head_dim or dout.numel() != out.numel() or lse.numel() != B * H * N:
        raise RuntimeError("attention_bwd: shapes do not match [B,N,H*hd] / [B,H,N]")
    dqkv = torch.empty_like(qkv)
    with _timed("attention_bwd", {"flops": 10.0 * B * H * N * N * head_dim}, qkv):
        rc = _lib.load().smoe_attention_bwd(_ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), _ptr(dqkv), dtype_code(qkv.dtype), B, N,
                                            H, head_dim, float(scale), _stream(qkv))
    _lib.check(rc, "smoe_attention_bwd")
    return dqkv


# ---- skip-aware attention half (eval): plan -> gathered qkv GEMM -> varlen attention -> projection with a row map -> expand ----
VARLEN_WEIGHT_SCORE, VARLEN_NO_TIERS = 1, 2   # flags of smoe_attention_fwd_varlen (include/slimmoe.h)
VARLEN_MAX_LEN = 256


def skip_attention_supported(N: int, head_dim: int) -> bool:
    """Shapes smoe_attention_fwd_varlen covers: the one-pass form (N <= 256), head dim 64."""
    return 1 <= N <= VARLEN_MAX_LEN and head_dim == 64


def skip_plan(mask: torch.Tensor, B: int, N: int, park: Optional[torch.Tensor] = None) -> dict:
    """The gate's mask (f32 [B*N, 2], channel 0 = bypassed) -> the device-side plan of the skip-aware attention half: per-image
    ``row_start`` / ``len`` / ``mult`` (i32 [B]), ``gather`` and ``row_map`` (i64 [B*N]), ``offsets`` (i32 [2] = [0, R]) and ``rep_row``
    (i32 [B*N]).  ``park`` (f32 [B, d]): the representatives' output rows behind the token matrix, zeroed by the same call.  The host
    never learns R."""
    _chk(mask, "mask", torch.float32, align=4)
    T = B * N
    if mask.numel() != T * 2 or B < 1 or N < 1:
        raise RuntimeError(f"mask: expected [B*N, 2] with B={B}, N={N}, got {tuple(mask.shape)}")
    cols = 0
    if park is not None:
        _chk(park, "park", torch.float32, 2, align=4)
        if park.shape[0] != B:
            raise RuntimeError(f"park: expected [{B}, d], got {tuple(park.shape)}")
        cols = park.shape[1]
    dev = mask.device
    i32 = torch.empty(4 + 3 * B + T, dtype=torch.int32, device=dev)      # one allocation for the small tables (offsets 16-byte aligned)
    offsets, row_start, length, mult, rep_row = i32[:2], i32[4:4 + B], i32[4 + B:4 + 2 * B], i32[4 + 2 * B:4 + 3 * B], i32[4 + 3 * B:]
    i64 = torch.empty(2 * T, dtype=torch.int64, device=dev)
    gather, row_map = i64[:T], i64[T:]
    with _timed("skip_plan", {"bytes": T * (8 + 16 + 4)}, mask):
        rc = _lib.load().smoe_skip_plan(_ptr(mask), B, N, _ptr(row_start), _ptr(length), _ptr(mult), _ptr(gather), _ptr(row_map),
                                        _ptr(offsets), _ptr(rep_row), _ptr(park), cols, _stream(mask))
    _lib.check(rc, "smoe_skip_plan")
    return {"row_start": row_start, "len": length, "mult": mult, "gather": gather, "row_map": row_map, "offsets": offsets,
            "rep_row": rep_row, "B": B, "N": N}


def attention_varlen(qkv: torch.Tensor, row_start: torch.Tensor, length: torch.Tensor, mult: torch.Tensor, max_len: int, H: int,
                     head_dim: int, scale: float, flags: int = 0) -> torch.Tensor:
    """softmax(q k^T * scale) v over the compact qkv [rows, 3*H*head_dim] (16 bit): image b owns the rows [row_start[b], row_start[b]
    + len[b]) and, with mult[b] > 0, its last key counts mult[b] times -> [rows, H*head_dim], the same compact rows (rows no image
    owns are not written).  ``max_len``: host-side bound on every len (<= 256)."""
    _chk(qkv, "qkv", ndim=2)
    if qkv.dtype not in (torch.float16, torch.bfloat16) or qkv.shape[1] != 3 * H * head_dim:
        raise RuntimeError("qkv: expected a 16-bit [rows, 3*H*hd] tensor")
    if not skip_attention_supported(max_len, head_dim):
        raise RuntimeError(f"attention_varlen: max_len={max_len}, head_dim={head_dim} outside the kernel's reach (<= 256, 64)")
    B = row_start.numel()
    for t, nm in ((row_start, "row_start"), (length, "len"), (mult, "mult")):
        _chk(t, nm, torch.int32, 1, align=4)
        if t.numel() != B:
            raise RuntimeError(f"{nm}: expected {B} entries")
    rows = qkv.shape[0]
    out = torch.empty((rows, H * head_dim), dtype=qkv.dtype, device=qkv.device)
    with _timed("attention_varlen", {"flops": 4.0 * B * H * max_len * max_len * head_dim}, qkv):
        rc = _lib.load().smoe_attention_fwd_varlen(_ptr(qkv), _ptr(out), dtype_code(qkv.dtype), _ptr(row_start), _ptr(length),
                                                   _ptr(mult), B, max_len, rows, H, head_dim, float(scale), int(flags), _stream(qkv))
    _lib.check(rc, "smoe_attention_fwd_varlen")
    return out


def skip_expand(xn32: torch.Tensor, rep_row: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """``out[t] = xn32[t] + out[rep_row[t]]`` for every token t with ``rep_row[t] >= 0`` (the bypassed ones); other rows of ``out``
    are untouched.  ``xn32`` [T, d] f32 may be the first T rows of ``out`` [>= T, d] itself."""
    _chk(xn32, "xn32", torch.float32, 2)
    _chk(out, "out", torch.float32, 2)
    _chk(rep_row, "rep_row", torch.int32, 1, align=4)
    T, d = xn32.shape
    if out.shape[1] != d or out.shape[0] < T or rep_row.numel() != T or d % 4:
        raise RuntimeError("skip_expand: expected xn32 [T, d], out [>= T, d], rep_row [T], d % 4 == 0")
    with _timed("skip_expand", {"bytes": 0}, out):
        rc = _lib.load().smoe_skip_expand(_ptr(xn32), _ptr(rep_row), _ptr(out), T, d, out.shape[0], _stream(out))
    _lib.check(rc, "smoe_skip_expand")
    return out


def ln_router_supported(d: int, E: int, k: int) -> bool:
    return bool(_lib.load().smoe_ln_router_supported(d, E, k))


# SLIMMOE_ROUTER_HIST=1: the fused router pass also counts for the dispatch plan (count_by_gate folded in: chunk_hist +
# smoe_dispatch_plan_hist, one plan launch instead of two).  Bit-identical plans, and OFF by default: measured inside the model
# (two alternating bench runs on one box) the LayerNorm + router pass costs 72.3-73.1 us with it against 68.9-69.2 us without (it must
# walk contiguous 64-token chunks: 788 workgroups of 4 groups instead of 631 of 5) while the plan only drops from 15.1-15.4 to
# 14.8 us -- the counting launch was nearly free next to the assign launch, which now reads a 16 x longer table.
ROUTER_HIST = _os.environ.get("SLIMMOE_ROUTER_HIST", "0") == "1"


def chunk_hist(T: int, d: int, E: int, k: int, device) -> Optional[torch.Tensor]:
    """An (uninitialised) chunk-histogram table for the fused router passes to fill -- i32 [ceil(T / tok), E] with ``.tok`` tokens
    per row -- or None when this shape's router writes none (dispatch_plan then counts by itself)."""
    if not ROUTER_HIST or T <= 0:
        return None
    tok = _lib.load().smoe_router_chunk_hist_tokens(d, E, k)
    if tok <= 0:
        return None
    t = torch.empty((-(-T // tok), E), dtype=torch.int32, device=device)
    t.tok = tok
    return t


def ln_router_topk(x: torch.Tensor, ln_weight: Optional[torch.Tensor], ln_bias: Optional[torch.Tensor], eps: float,
                   wg: torch.Tensor, bg: Optional[torch.Tensor], k: int, gate_kind: int = GATE_NAIVE,
                   noise: Optional[torch.Tensor] = None, xn16_dtype: Optional[torch.dtype] = torch.float16,
                   want_xn32: bool = False, want_probs: bool = False, want_logits: bool = False, force_f64: bool = False,
                   hist: Optional[torch.Tensor] = None):
    """LayerNorm + router in one pass: (xn16 | None, xn32 | None, idx, score, logits | None, probs | None).  ``hist``
    (chunk_hist(T, d, E, k, device)): filled with the routing's per-chunk expert counts for dispatch_plan(hist=...)."""
    _chk(x, "x", ndim=2)
    _chk(wg, "wg", torch.float32, 2)
    T, d = x.shape
    E = wg.shape[0]
    for t, nm in ((ln_weight, "ln_weight"), (ln_bias, "ln_bias"), (bg, "bg")):
        if t is not None:
            _chk(t, nm, torch.float32, 1)
    dev = x.device
    xn16 = torch.empty((T, d), dtype=xn16_dtype, device=dev) if xn16_dtype is not None else None
    xn32 = torch.empty((T, d), dtype=torch.float32, device=dev) if want_xn32 else None
    idx = torch.empty((T, k), dtype=torch.int64, device=dev)
    score = torch.empty((T, k), dtype=torch.float32, device=dev)
    logits = torch.empty((T, E), dtype=torch.float32, device=dev) if want_logits else None
    probs = torch.empty((T, E), dtype=torch.float32, device=dev) if want_probs else None
    lib = _lib.load()
    ws, ws_bytes, flags = _router_call_workspace(dev, T, force_f64)
    nbytes = T * d * (x.element_size() + (2 if xn16 is not None else 0) + (4 if want_xn32 else 0))
    with _timed("ln_router", {"bytes": nbytes}, x):
        rc = lib.smoe_ln_router_topk(_ptr(x), dtype_code(x.dtype), _ptr(ln_weight), _ptr(ln_bias), float(eps), _ptr(xn16),
                                     dtype_code(xn16_dtype) if xn16_dtype is not None else F16, _ptr(xn32), _ptr(wg),
                                     _ptr(bg), _ptr(noise), T, d, E, k, gate_kind | flags,
                                     _ptr(idx), _ptr(score), _ptr(logits), _ptr(probs), _ptr(None if force_f64 else hist), _ptr(ws),
                                     ws_bytes, _stream(x))
    _lib.check(rc, "smoe_ln_router_topk")
    return xn16, xn32, idx, score, logits, probs


def gate_ln_router_supported(d: int, E: int, k: int) -> bool:
    return bool(_lib.load().smoe_gate_ln_router_supported(d, E, k))


def gate_ln_router(x: torch.Tensor, gate_w: torch.Tensor, gate_b: Optional[torch.Tensor], threshold: Optional[torch.Tensor],
                   ln: Optional[tuple] = None, wg: Optional[torch.Tensor] = None, bg: Optional[torch.Tensor] = None,
                   k: int = 1, xn16_dtype: Optional[torch.dtype] = None, want_xn32: bool = False,
                   zero_out: Optional[torch.Tensor] = None, want_mask: bool = False,
                   skip_count: Optional[torch.Tensor] = None, xn32_out: Optional[torch.Tensor] = None,
                   hist: Optional[torch.Tensor] = None, want_tk32: bool = False):
    """[LayerNorm +] token-skip gate (+ NaiveGate router) in one pass (smoe_gate_ln_router).  ``ln`` = (weight, bias,
    eps) or None; ``threshold`` = the gate's 0-dim DEVICE buffer (None = gate disabled); ``wg`` None = no router.
    Returns a dict: xn16, xn32, idx, idx_plan, score, mask, tk32 (entries that were not asked for are None); ``tk32`` = the f32 row
    with zeros for the skipped tokens (``want_tk32``)."""
    _chk(x, "x", torch.float32, 2)
    T, d = x.shape
    dev = x.device
    gw = gate_w.detach().reshape(-1)
    _chk(gw, "gate_w", torch.float32, 1, align=4)
    if gw.numel() != d:
        raise RuntimeError(f"gate_w: expected {d} elements")
    gb = gate_b.detach().reshape(-1) if gate_b is not None else None
    thr = threshold.detach().reshape(-1) if threshold is not None else None
    for t, nm in ((gb, "gate_b"), (thr, "threshold")):
        if t is not None:
            _chk(t, nm, torch.float32, 1, align=4)
    E = 0
    if wg is not None:
        _chk(wg, "wg", torch.float32, 2)
        E = wg.shape[0]
        if bg is not None:
            _chk(bg, "bg", torch.float32, 1, align=4)
    lg = lb = None
    eps = 0.0
    if ln is not None:
        lg, lb, eps = ln
        for t, nm in ((lg, "ln_weight"), (lb, "ln_bias")):
            if t is not None:
                _chk(t, nm, torch.float32, 1)
    if zero_out is not None:
        _chk(zero_out, "zero_out", torch.float32, 1)
    xn16 = torch.empty((T, d), dtype=xn16_dtype, device=dev) if xn16_dtype is not None else None
    xn32 = xn32_out if xn32_out is not None else (torch.empty((T, d), dtype=torch.float32, device=dev) if want_xn32 else None)
    if xn32 is not None:
        _chk(xn32, "xn32", torch.float32, 2)
    idx = torch.empty((T, k), dtype=torch.int64, device=dev) if E else None
    idx_plan = torch.empty((T, k), dtype=torch.int64, device=dev) if E else None
    score = torch.empty((T, k), dtype=torch.float32, device=dev) if E else None
    mask = torch.empty((T, 2), dtype=torch.float32, device=dev) if want_mask else None
    tk32 = torch.empty((T, d), dtype=torch.float32, device=dev) if want_tk32 else None
    if skip_count is not None:
        _chk(skip_count, "skip_count", torch.int32, align=4)
    lib = _lib.load()
    ws, ws_bytes, flags = _router_call_workspace(dev, T)
    with_ln = (GATE_WITH_LN if ln is not None else 0) | (GATE_WS_KEPT_ZERO if flags & WS_KEPT_ZERO else 0)
    nbytes = T * d * (4 + (2 if xn16 is not None else 0) + (4 if xn32 is not None else 0) + (4 if tk32 is not None else 0))
    with _timed("gate_ln_router" if E else "gate_ln", {"bytes": nbytes}, x):
        rc = lib.smoe_gate_ln_router(_ptr(x), F32, with_ln, _ptr(lg), _ptr(lb), float(eps), _ptr(gw),
                                     _ptr(gb), _ptr(thr), _ptr(xn16),
                                     dtype_code(xn16_dtype) if xn16_dtype is not None else F16, _ptr(xn32),
                                     _ptr(zero_out), _ptr(wg), _ptr(bg), T, d, E, k, _ptr(idx), _ptr(idx_plan),
                                     _ptr(score), _ptr(mask), _ptr(skip_count), _ptr(hist if E else None), _ptr(tk32), _ptr(ws),
                                     ws_bytes, _stream(x))
    _lib.check(rc, "smoe_gate_ln_router")
    return {"xn16": xn16, "xn32": xn32, "idx": idx, "idx_plan": idx_plan, "score": score, "mask": mask, "tk32": tk32}


def soft_gate_ln_supported(d: int) -> bool:
    return bool(_lib.load().smoe_soft_gate_ln_fwd_supported(d))


def soft_gate_ln(x: torch.Tensor, gate_w: torch.Tensor, gate_b: Optional[torch.Tensor], ln: Optional[tuple] = None,
                 xn16_dtype: Optional[torch.dtype] = None, want_xn32: bool = False, want_tk32: bool = False,
                 want_mask: bool = False, skip_count: Optional[torch.Tensor] = None):
    """[LayerNorm +] SOFT token-skip gate in one pass (smoe_soft_gate_ln_fwd): p = sigmoid(<xn, gate_w> + gate_b), tk = xn * p.
    ``ln`` = (weight, bias, eps) or None.  Returns gate_ln_router's dict shape: xn32 (the normed rows), xn16 (the 16-bit image of
    ``tk``, ``xn16_dtype``), tk32 (the f32 image of ``tk``), mask = (1 - p, p) (entries that were not asked for are None; idx /
    idx_plan / score are always None: nothing is routed here).  ``skip_count`` (int32[1]) grows by rint(sum (1 - p))."""
    _chk(x, "x", torch.float32, 2)
    T, d = x.shape
    dev = x.device
    if not soft_gate_ln_supported(d):
        raise RuntimeError(f"soft_gate_ln: unsupported d={d} (192, 384, 768, 1024)")
    gw = gate_w.detach().reshape(-1)
    _chk(gw, "gate_w", torch.float32, 1)
    if gw.numel() != d:
        raise RuntimeError(f"gate_w: expected {d} elements")
    gb = gate_b.detach().reshape(-1) if gate_b is not None else None
    if gb is not None:
        _chk(gb, "gate_b", torch.float32, 1, align=4)
    lg = lb = None
    eps = 0.0
    if ln is not None:
        lg, lb, eps = ln
        for t, nm in ((lg, "ln_weight"), (lb, "ln_bias")):
            if t is not None:
                _chk(t, nm, torch.float32, 1)
                if t.numel() != d:
                    raise RuntimeError(f"{nm}: expected {d} elements")
    if xn16_dtype is not None and xn16_dtype not in (torch.float16, torch.bfloat16):
        raise TypeError("soft_gate_ln: xn16_dtype must be float16 or bfloat16")
    xn16 = torch.empty((T, d), dtype=xn16_dtype, device=dev) if xn16_dtype is not None else None
    xn32 = torch.empty((T, d), dtype=torch.float32, device=dev) if want_xn32 else None
    tk32 = torch.empty((T, d), dtype=torch.float32, device=dev) if want_tk32 else None
    mask = torch.empty((T, 2), dtype=torch.float32, device=dev) if want_mask else None
    lib = _lib.load()
    ws, ws_bytes = None, 0
    if skip_count is not None:
        _chk(skip_count, "skip_count", torch.int32, align=4)
        ws_bytes = lib.smoe_soft_gate_ln_fwd_workspace_bytes(T)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)   # (<= 8 KB: one partial sum per workgroup)
    nbytes = T * d * (4 + (2 if xn16 is not None else 0) + (4 if xn32 is not None else 0) + (4 if tk32 is not None else 0))
    with _timed("soft_gate_ln", {"bytes": nbytes}, x):
        rc = lib.smoe_soft_gate_ln_fwd(_ptr(x), F32, GATE_WITH_LN if ln is not None else 0, _ptr(lg), _ptr(lb), float(eps), _ptr(gw),
                                       _ptr(gb), _ptr(xn32), _ptr(xn16), dtype_code(xn16_dtype) if xn16_dtype is not None else F16,
                                       _ptr(tk32), _ptr(mask), _ptr(skip_count), T, d, _ptr(ws), ws_bytes, _stream(x))
    _lib.check(rc, "smoe_soft_gate_ln_fwd")
    return {"xn16": xn16, "xn32": xn32, "idx": None, "idx_plan": None, "score": None, "mask": mask, "tk32": tk32}


def _gate_mode(gate_on) -> int:
    """gate_on of the two gate backward entry points: False / 0 = disabled, True / 1 = hard (straight-through), 2 = soft."""
    if isinstance(gate_on, bool):
        return 1 if gate_on else 0
    if isinstance(gate_on, int) and gate_on in (0, 1, 2):
        return gate_on
    raise ValueError(f"gate_on: expected False / True or 0 (disabled), 1 (hard), 2 (soft), got {gate_on!r}")


def gate_ln_bwd(x: torch.Tensor, g_f: torch.Tensor, g_out: Optional[torch.Tensor], ln_w: Optional[torch.Tensor],
                ln_b: Optional[torch.Tensor], eps: float, gate_w: torch.Tensor, gate_b: Optional[torch.Tensor],
                mask: Optional[torch.Tensor], gate_on=True, want_dz: bool = False):
    """Backward of one gated half's front end (LayerNorm -> token-skip gate) in one pass over its input x (smoe_gate_ln_bwd):
    (dx f32 [T,d], dln_w [d], dln_b [d], dgate_w [d], dgate_b [1], dz [T] | None).  ``gate_on``: False / True as before, or 2 = the
    soft gate (``mask`` = soft_gate_ln's (1 - p, p); dz takes the positive sign)."""
    gate_on = _gate_mode(gate_on)
    _chk(x, "x", torch.float32, 2)
    _chk(g_f, "g_f", ndim=2)
    T, d = x.shape
    if tuple(g_f.shape) != (T, d):
        raise RuntimeError("gate_ln_bwd: g_f must have x's shape")
    if g_out is not None:
        _chk(g_out, "g_out", torch.float32, 2)
    gw = gate_w.detach().reshape(-1)
    _chk(gw, "gate_w", torch.float32, 1, align=4)
    gb = gate_b.detach().reshape(-1) if gate_b is not None else None
    if gb is not None:
        _chk(gb, "gate_b", torch.float32, 1, align=4)
    if mask is not None:
        _chk(mask, "mask", torch.float32, 2, align=4)
    for nm, t in (("ln_w", ln_w), ("ln_b", ln_b)):
        if t is not None:
            _chk(t, nm, torch.float32, 1)
    lib = _lib.load()
    dx = torch.empty_like(x)
    out = torch.empty(3 * d + 4, dtype=torch.float32, device=x.device)
    dz = torch.empty(T, dtype=torch.float32, device=x.device) if want_dz else None
    ws_bytes = lib.smoe_gate_ln_bwd_workspace_bytes(T, d)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    rc = lib.smoe_gate_ln_bwd(_ptr(x), _ptr(g_f), dtype_code(g_f.dtype), _ptr(g_out), _ptr(ln_w), _ptr(ln_b), float(eps), _ptr(gw),
                              _ptr(gb), _ptr(mask), gate_on, T, d, _ptr(dx), _ptr(dz), _ptr(out), _ptr(ws), ws_bytes,
                              _stream(x))
    _lib.check(rc, "smoe_gate_ln_bwd")
    return dx, out[:d], out[d:2 * d], out[2 * d:3 * d], out[3 * d:3 * d + 1], dz


def skip_gate_bwd(xn: torch.Tensor, g_f: torch.Tensor, g_out: Optional[torch.Tensor], gate_w: torch.Tensor,
                  gate_b: Optional[torch.Tensor], mask: Optional[torch.Tensor], gate_on=True):
    """Backward of one gated half of the residual-MoE block in training (smoe_skip_gate_bwd): (dxn f32 [T,d], dz f32 [T]).
    ``gate_on`` as in gate_ln_bwd (2 = the soft gate)."""
    gate_on = _gate_mode(gate_on)
    _chk(xn, "xn", torch.float32, 2)
    _chk(g_f, "g_f", ndim=2)
    T, d = xn.shape
    if tuple(g_f.shape) != (T, d):
        raise RuntimeError("skip_gate_bwd: g_f must have xn's shape")
    if g_out is not None:
        _chk(g_out, "g_out", torch.float32, 2)
    gw = gate_w.detach().reshape(-1)
    _chk(gw, "gate_w", torch.float32, 1, align=4)
    gb = gate_b.detach().reshape(-1) if gate_b is not None else None
    if mask is not None:
        _chk(mask, "mask", torch.float32, 2, align=4)
    dxn = torch.empty_like(xn)
    dz = torch.empty(T, dtype=torch.float32, device=xn.device)
    rc = _lib.load().smoe_skip_gate_bwd(_ptr(xn), _ptr(g_f), dtype_code(g_f.dtype), _ptr(g_out), _ptr(gw), _ptr(gb), _ptr(mask),
                                        gate_on, T, d, _ptr(dxn), _ptr(dz), _stream(xn))
    _lib.check(rc, "smoe_skip_gate_bwd")
    return dxn, dz


def zero_row_output(bg: Optional[torch.Tensor], k: int, w2: torch.Tensor, b1: Optional[torch.Tensor],
                    b2: Optional[torch.Tensor], e_base: int = 0, E_total: Optional[int] = None) -> torch.Tensor:
    """out[d] = sum_j score_j (W2[e_j] gelu(b1[e_j]) + b2[e_j]) for the NaiveGate routing of an all-zero row.  Expert parallel
    (``E_total`` global experts in ``bg``, ``w2`` / ``b1`` / ``b2`` = this rank's experts [e_base, e_base + E_local)): this rank's
    partial sum -- the ranks' results add up to the row."""
    _chk(w2, "w2", torch.float32, 3)
    E_local, d, h = w2.shape
    E = E_local if E_total is None else int(E_total)
    for t, nm in ((bg, "bg"), (b1, "b1"), (b2, "b2")):
        if t is not None:
            _chk(t, nm, torch.float32, align=4)
    if bg is not None and bg.numel() != E:
        raise RuntimeError(f"zero_row_output: bg has {bg.numel()} entries, expected {E}")
    out = torch.empty(d, dtype=torch.float32, device=w2.device)
    rc = _lib.load().smoe_zero_row_output(_ptr(bg), E, k, _ptr(w2), _ptr(b1), _ptr(b2), d, h, int(e_base), E_local, _ptr(out),
                                          _stream(w2))
    _lib.check(rc, "smoe_zero_row_output")
    return out


def dispatch_plan(idx: torch.Tensor, E: int, capacity: int = -1, want_pruned: Optional[bool] = None,
                  hist: Optional[torch.Tensor] = None, subset: Optional[tuple] = None):
    """(counts i32 [E], offsets i32 [E+1], pos i64 [n], inv_pos i64 [n], idx_pruned i64 [n] | None).  ``hist``: the chunk histogram the
    fused router filled for exactly this ``idx`` (chunk_hist / ln_router_topk / gate_ln_router): the plan then skips its counting
    launch (smoe_dispatch_plan_hist).  ``subset`` = (period, prefix) in tokens: only the tokens t with t % period < prefix are
    dispatched (smoe_dispatch_plan_subset; no capacity, and a router histogram -- it counted every token -- is not used): the
    first ``offsets[E]`` entries of ``pos`` hold their flat entries, expert by expert, and ``inv_pos`` is -1 everywhere else."""
    _chk(idx, "idx", torch.int64, align=8)  # read element-wise: slices of a [T,k] tensor are fine
    flat = idx.reshape(-1)
    n = flat.numel()
    dev = idx.device
    if want_pruned is None:
        want_pruned = capacity >= 0
    lib = _lib.load()
    ws_bytes = lib.smoe_dispatch_plan_workspace_bytes(n, E)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(E, dtype=torch.int32, device=dev)
    offsets = torch.empty(E + 1, dtype=torch.int32, device=dev)
    pos = torch.empty(n, dtype=torch.int64, device=dev)
    inv_pos = torch.empty(n, dtype=torch.int64, device=dev)
    pruned = torch.empty(n, dtype=torch.int64, device=dev) if want_pruned else None
    if subset is not None:
        period, prefix = int(subset[0]), int(subset[1])
        if capacity >= 0 or want_pruned or not 0 <= prefix <= period:
            raise RuntimeError(f"dispatch_plan: subset=({period}, {prefix}) needs capacity < 0 (no idx_pruned) and 0 <= prefix <= period")
        kk = idx.shape[1] if idx.dim() == 2 else 1          # flat entries per token
    with _timed("plan", {"bytes": n * 24}, idx):
        if subset is not None:
            rc = lib.smoe_dispatch_plan_subset(_ptr(flat), n, E, period * kk, prefix * kk, _ptr(counts), _ptr(offsets), _ptr(pos),
                                               _ptr(inv_pos), _ptr(ws), ws_bytes, _stream(idx))
        elif hist is not None:
            _chk(hist, "hist", torch.int32, 2)
            k = idx.shape[1] if idx.dim() == 2 else 1      # flat entries per token
            rc = lib.smoe_dispatch_plan_hist(_ptr(flat), n, E, int(capacity), _ptr(hist), int(hist.tok) * k, _ptr(counts), _ptr(offsets),
                                             _ptr(pos), _ptr(inv_pos), _ptr(pruned), _ptr(ws), ws_bytes, _stream(idx))
        else:
            rc = lib.smoe_dispatch_plan(_ptr(flat), n, E, int(capacity), _ptr(counts), _ptr(offsets), _ptr(pos),
                                        _ptr(inv_pos), _ptr(pruned), _ptr(ws), ws_bytes, _stream(idx))
    _lib.check(rc, "smoe_dispatch_plan")
    return counts, offsets, pos, inv_pos, pruned


def dispatch_plan_padded(idx: torch.Tensor, E: int, capacity: int, slot_rows: Optional[int] = None, want_raw: bool = False):
    """The plan in the padded layout of a capacity gate's static exchange: expert e owns the slots [e * slot_rows, (e + 1) *
    slot_rows) (slot_rows >= capacity, default = capacity).  Returns (counts i32 [E], offsets i32 [E+1] (compact prefix),
    group_end i32 [E] = e * slot_rows + counts[e], pos_padded i64 [E * slot_rows] (-1 = unused slot), inv_pos i64 [n] (padded
    slot or -1), idx_pruned i64 [n]); with ``want_raw`` a seventh entry, raw_counts i32 [E] = the entries routed to each expert
    before the capacity clamp."""
    slot_rows = int(capacity) if slot_rows is None else int(slot_rows)
    _chk(idx, "idx", torch.int64, align=8)
    flat = idx.reshape(-1)
    n = flat.numel()
    dev = idx.device
    lib = _lib.load()
    ws_bytes = lib.smoe_dispatch_plan_workspace_bytes(n, E)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(E, dtype=torch.int32, device=dev)
    offsets = torch.empty(E + 1, dtype=torch.int32, device=dev)
    group_end = torch.empty(E, dtype=torch.int32, device=dev)
    pos = torch.empty(E * slot_rows, dtype=torch.int64, device=dev)
    inv_pos = torch.empty(n, dtype=torch.int64, device=dev)
    pruned = torch.empty(n, dtype=torch.int64, device=dev)
    raw = torch.empty(E, dtype=torch.int32, device=dev) if want_raw else None
    with _timed("plan", {"bytes": n * 24}, idx):
        rc = lib.smoe_dispatch_plan_padded(_ptr(flat), n, E, int(capacity), slot_rows, _ptr(counts), _ptr(offsets), _ptr(group_end),
                                           _ptr(pos), _ptr(inv_pos), _ptr(pruned), _ptr(raw), _ptr(ws), ws_bytes, _stream(idx))
    _lib.check(rc, "smoe_dispatch_plan_padded")
    if want_raw:
        return counts, offsets, group_end, pos, inv_pos, pruned, raw
    return counts, offsets, group_end, pos, inv_pos, pruned


def dispatch_plan_slots(idx: torch.Tensor, E: int, slot_base: torch.Tensor, n_slots: int, capacity: int = -1, hdr_rows: int = 1):
    """The plan over a slot table (smoe_dispatch_plan_slots): expert e owns the slots [slot_base[e], slot_base[e + 1]) (i32 [E + 1] on
    the device; ``n_slots`` = slot_base[E], known to the host), the last ``hdr_rows`` of them reserved.  Returns (counts i32 [E],
    offsets i32 [E+1], group_end i32 [E], pos_slots i64 [n_slots] (-1 = unused), inv_pos i64 [n], idx_pruned i64 [n],
    raw_counts i32 [E] = the entries routed to each expert before any clamp)."""
    _chk(idx, "idx", torch.int64, align=8)
    _chk(slot_base, "slot_base", torch.int32, 1, align=4)
    if slot_base.numel() != E + 1:
        raise RuntimeError("slot_base: expected E + 1 entries")
    flat = idx.reshape(-1)
    n = flat.numel()
    dev = idx.device
    lib = _lib.load()
    ws_bytes = lib.smoe_dispatch_plan_workspace_bytes(n, E)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(E, dtype=torch.int32, device=dev)
    offsets = torch.empty(E + 1, dtype=torch.int32, device=dev)
    group_end = torch.empty(E, dtype=torch.int32, device=dev)
    pos = torch.empty(int(n_slots), dtype=torch.int64, device=dev)
    inv_pos = torch.empty(n, dtype=torch.int64, device=dev)
    pruned = torch.empty(n, dtype=torch.int64, device=dev)
    raw = torch.empty(E, dtype=torch.int32, device=dev)
    with _timed("plan", {"bytes": n * 24}, idx):
        rc = lib.smoe_dispatch_plan_slots(_ptr(flat), n, E, int(capacity), _ptr(slot_base), int(hdr_rows), _ptr(counts), _ptr(offsets),
                                          _ptr(group_end), _ptr(pos), _ptr(inv_pos), _ptr(pruned), _ptr(raw), _ptr(ws), ws_bytes,
                                          _stream(idx))
    _lib.check(rc, "smoe_dispatch_plan_slots")
    return counts, offsets, group_end, pos, inv_pos, pruned, raw


def ep_pack_headers(send: torch.Tensor, counts: Optional[torch.Tensor], raw_counts: Optional[torch.Tensor], slot_base: torch.Tensor,
                    t_rows: int) -> None:
    """Write the header rows of a static-exchange send buffer (smoe_ep_pack_headers): region g's last row gets int32
    {counts[g], raw_counts[g], t_rows, G, raw_counts[0 .. G)}."""
    _chk(send, "send", ndim=2)
    _chk(slot_base, "slot_base", torch.int32, 1, align=4)
    G = slot_base.numel() - 1
    for t, nm in ((counts, "counts"), (raw_counts, "raw_counts")):
        if t is not None:
            _chk(t, nm, torch.int32, 1, align=4)
            if t.numel() != G:
                raise RuntimeError(f"{nm}: expected {G} entries")
    rc = _lib.load().smoe_ep_pack_headers(_ptr(counts), _ptr(raw_counts), _ptr(slot_base), G, send.shape[1] * send.element_size(),
                                          int(t_rows), _ptr(send), _stream(send))
    _lib.check(rc, "smoe_ep_pack_headers")


def ep_unpack_headers(recv: torch.Tensor, W: int, local_base: torch.Tensor, E_total: int):
    """(starts i32 [G], ends i32 [G], stats i32 [W, 1 + E_total]) from the header rows of a received static-exchange buffer
    (smoe_ep_unpack_headers): group l = (source rank, local expert) holds the rows [starts[l], ends[l]); stats[w] = (source w's
    row count, its pre-clamp counts of all E_total experts)."""
    _chk(recv, "recv", ndim=2)
    _chk(local_base, "local_base", torch.int32, 1, align=4)
    E_local = local_base.numel() - 1
    G = int(W) * E_local
    dev = recv.device
    starts = torch.empty(G, dtype=torch.int32, device=dev)
    ends = torch.empty(G, dtype=torch.int32, device=dev)
    stats = torch.empty((int(W), 1 + int(E_total)), dtype=torch.int32, device=dev)
    rc = _lib.load().smoe_ep_unpack_headers(_ptr(recv), int(W), E_local, _ptr(local_base), recv.shape[1] * recv.element_size(),
                                            int(E_total), _ptr(starts), _ptr(ends), _ptr(stats), _stream(recv))
    _lib.check(rc, "smoe_ep_unpack_headers")
    return starts, ends, stats


def scatter_rows(x: torch.Tensor, pos: torch.Tensor, k: int, out_dtype: torch.dtype,
                 out: Optional[torch.Tensor] = None, zero_fill: bool = False,
                 scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """buf[s] = cast(x[pos[s] // k]) (* scale[pos[s]]) for every slot with pos[s] >= 0 (MOEScatter local part;
    with ``scale`` = the adjoint of the combine); ``zero_fill``: the other slots become zero rows (also of a given ``out``)."""
    _chk(x, "x", ndim=2)
    _chk(pos, "pos", torch.int64, 1, align=8)
    n_slots = pos.numel()
    d = x.shape[1]
    if out is None:
        out = torch.empty((n_slots, d), dtype=out_dtype, device=x.device)
    else:
        _chk(out, "out", out_dtype, 2)
    if scale is not None:
        _chk(scale, "scale", torch.float32, align=4)
        if scale.numel() != x.shape[0] * k:
            raise RuntimeError("scale: expected T*k entries")
    lib = _lib.load()
    # zero_fill: slots no token maps to (pos < 0) are written as zero rows by the same pass, not by a memset of the whole buffer
    fn = lib.smoe_scatter_rows_fill if zero_fill else lib.smoe_scatter_rows
    with _timed("scatter", {"bytes": n_slots * d * (x.element_size() + out.element_size())}, x):
        rc = fn(_ptr(x), dtype_code(x.dtype), _ptr(pos), _ptr(scale), n_slots, k, d, _ptr(out), dtype_code(out.dtype), _stream(x))
    _lib.check(rc, "smoe_scatter_rows")
    return out


def gather_combine(y: torch.Tensor, inv_pos: torch.Tensor, score: torch.Tensor, T: int, k: int,
                   out_dtype: torch.dtype, residual: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[t] = sum_j score[t,j] * y[inv_pos[t*k+j]] (+ residual[t]); dropped entries contribute 0."""
    _chk(y, "y", ndim=2)
    _chk(inv_pos, "inv_pos", torch.int64, align=8)
    _chk(score, "score", torch.float32, align=4)
    d = y.shape[1]
    if inv_pos.numel() != T * k or score.numel() != T * k:
        raise RuntimeError("inv_pos / score: expected T*k entries")
    if out is None:
        out = torch.empty((T, d), dtype=out_dtype, device=y.device)
    else:
        _chk(out, "out", out_dtype, 2)
        if tuple(out.shape) != (T, d):
            raise RuntimeError("out: expected [T,d]")
    if residual is not None:
        _chk(residual, "residual", out_dtype, 2)
    lib = _lib.load()
    with _timed("combine", {"bytes": T * d * (k * y.element_size() + out.element_size())}, y):
        rc = lib.smoe_gather_combine(_ptr(y), dtype_code(y.dtype), _ptr(inv_pos), _ptr(score), T, k, d, _ptr(residual),
                                     _ptr(out), dtype_code(out_dtype), _stream(y))
    _lib.check(rc, "smoe_gather_combine")
    return out


def gather_combine_ln(y: torch.Tensor, inv_pos: torch.Tensor, score: torch.Tensor, T: int, k: int,
                      residual: Optional[torch.Tensor], ln_weight: torch.Tensor, ln_bias: torch.Tensor, eps: float,
                      xn_dtype: torch.dtype = torch.float16, out: Optional[torch.Tensor] = None,
                      xn: Optional[torch.Tensor] = None):
    """(out f32 [T,d], xn [T,d] 16-bit): out[t] = residual[t] + sum_j score[t,j] y[inv_pos[t k + j]]; xn = LayerNorm(out).
    ``out`` / ``xn``: write into these (row slices of a layer's buffers: one call per token chunk)."""
    _chk(y, "y", ndim=2)
    _chk(inv_pos, "inv_pos", torch.int64, align=8)
    _chk(score, "score", torch.float32, align=4)
    _chk(ln_weight, "ln_weight", torch.float32, 1)
    _chk(ln_bias, "ln_bias", torch.float32, 1)
    d = y.shape[1]
    if residual is not None:
        _chk(residual, "residual", torch.float32, 2)
    if out is None:
        out = torch.empty((T, d), dtype=torch.float32, device=y.device)
    else:
        _chk(out, "out", torch.float32, 2)
    if xn is None:
        xn = torch.empty((T, d), dtype=xn_dtype, device=y.device)
    else:
        _chk(xn, "xn", xn_dtype, 2)
    if tuple(out.shape) != (T, d) or tuple(xn.shape) != (T, d):
        raise RuntimeError("gather_combine_ln: out / xn must be [T, d]")
    with _timed("combine_ln", {"bytes": T * d * (k * y.element_size() + 8 + 2)}, y):
        rc = _lib.load().smoe_gather_combine_ln(_ptr(y), dtype_code(y.dtype), _ptr(inv_pos), _ptr(score), T, k, d, _ptr(residual),
                                                _ptr(out), _ptr(ln_weight), _ptr(ln_bias), float(eps), _ptr(xn), dtype_code(xn_dtype),
                                                _stream(y))
    _lib.check(rc, "smoe_gather_combine_ln")
    return out, xn


_reserved_cus = 0


def set_reserved_cus(n: int) -> int:
    """The persistent grouped GEMM leaves ``n`` CUs free from now on (smoe_set_reserved_cus; process-wide): kernels on other streams
    -- RCCL's all-to-all under the expert-parallel micro-batch pipeline -- can then run BESIDE the GEMMs instead of behind them.
    Returns the previous value.  Results do not depend on it."""
    global _reserved_cus
    _lib.check(_lib.load().smoe_set_reserved_cus(int(n)), "smoe_set_reserved_cus")
    prev, _reserved_cus = _reserved_cus, int(n)
    return prev


def grouped_gemm(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], offsets: torch.Tensor,
                 epilogue: int = EPI_NONE, out_dtype: Optional[torch.dtype] = None,
                 row_map: Optional[torch.Tensor] = None, row_scale: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, variant: int = 0,
                 group_expert: Optional[torch.Tensor] = None, rows_hint: Optional[int] = None,
                 residual: Optional[torch.Tensor] = None, a_gather: Optional[torch.Tensor] = None,
                 a_div: int = 1, prof_name: str = "grouped_gemm", group_end: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = epi(A[r] @ W[e]^T + bias[e]) for r in [offsets[g], offsets[g+1]), e = group_expert[g] (or g).
    W [E,N,K].  ``rows_hint`` = number of rows actually routed (for the profiler's FLOP count only).
    ``group_end`` (i32 [G]): separate row ranges [offsets[g], group_end[g]) -- ``offsets`` then has G entries (the padded
    buffers of a capacity gate's static exchange; persistent kernel only)."""
    _chk(A, "A", ndim=2)
    _chk(W, "W", A.dtype, 3)
    _chk(offsets, "offsets", torch.int32, 1)
    M, K = A.shape
    if a_gather is not None:  # A is the un-permuted token matrix; the GEMM has one row per routed slot
        _chk(a_gather, "a_gather", torch.int64, 1, align=8)
        M = a_gather.numel()
    E, N, K2 = W.shape
    if K2 != K:
        raise RuntimeError(f"W: expected [E,N,{K}], got {tuple(W.shape)}")
    G = offsets.numel() - 1
    if group_end is not None:
        _chk(group_end, "group_end", torch.int32, 1)
        G = offsets.numel()
        if group_end.numel() != G:
            raise RuntimeError("group_end: expected one entry per row group (offsets then holds the G starts)")
    if group_expert is None:
        if G != E:
            raise RuntimeError("offsets: expected E+1 entries")
    else:
        _chk(group_expert, "group_expert", torch.int32, 1)
        if group_expert.numel() != G:
            raise RuntimeError("group_expert: expected one entry per row group")
    if bias is not None:
        _chk(bias, "bias", torch.float32, 2)
        if tuple(bias.shape) != (E, N):
            raise RuntimeError("bias: expected [E,N]")
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else A.dtype
    if row_map is not None:
        _chk(row_map, "row_map", torch.int64, 1, align=8)
        if out is None:
            raise RuntimeError("row_map needs a caller-provided `out`")
        if row_scale is not None:
            _chk(row_scale, "row_scale", torch.float32, align=4)
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=A.device)
    else:
        _chk(out, "out", out_dtype, 2)
        if out.shape[1] != N:
            raise RuntimeError("out: expected N columns")
    if residual is not None:
        _chk(residual, "residual", out_dtype, 2)
        if tuple(residual.shape) != tuple(out.shape):
            raise RuntimeError("residual: expected the shape of out")
    lib = _lib.load()
    rows = M if rows_hint is None else rows_hint
    if a_gather is not None and 9 <= variant <= 14 and A.numel() * A.element_size() >= 2 ** 32:
        # the persistent kernel addresses A with 32-bit BYTE offsets and the library sees a_gather.numel() rows, not A's: a gathered
        # row of an A of 4 GiB or more would be read modulo 2^32.  The same plan runs in the one-workgroup-per-tile family
        # (64-bit row pointers), as the library itself chooses for an ungathered A of that size.
        if group_end is not None:
            raise RuntimeError("grouped_gemm: group_end needs the persistent kernel, and with a_gather that kernel needs all of A "
                               f"under 4 GiB (A is {tuple(A.shape)} {A.dtype})")
        variant = 4 if variant in (9, 14) else variant - 5
    if variant == 9 and group_end is not None and rows_hint is not None:
        # separate row ranges inside a PADDED buffer: the library picks tile height from the rows it is told about (M = the buffer);
        # ask it for its rule's answer (as an explicit variant, 10-13) for the rows that are expected to exist
        variant = lib.smoe_grouped_gemm_plan(int(rows_hint), G, K, N)
    with _timed(prof_name, {"flops": 2.0 * rows * K * N, "K": K, "N": N, "epilogue": epilogue}, A):
        rc = lib.smoe_grouped_gemm(_ptr(A), _ptr(W), _ptr(bias), _ptr(offsets), _ptr(group_expert), G, E, M, K, N,
                                   dtype_code(A.dtype), epilogue, _ptr(row_map), _ptr(row_scale), _ptr(residual),
                                   _ptr(a_gather), a_div, _ptr(out), out.shape[0], dtype_code(out_dtype), variant,
                                   _ptr(group_end), _stream(A))
    _lib.check(rc, "smoe_grouped_gemm")
    return out


# SLIMMOE_FFN_FUSED=1: one persistent launch for both expert GEMMs of a layer (smoe_expert_ffn).  Bit-identical to the two launches
# and OFF by default: measured 0.530-0.545 ms against 0.50-0.51 ms for the two launches at ViT-B / 256 images -- what the shared
# tile list saves in partly filled rounds (~30 us) goes into the switches between the two GEMM bodies, the write-through stores
# of H and the waits on late m-tiles (profiles/r04_fused_ffn.md).
# Since round 5 the launch is not in the default build: `make -C slim-switch-moe-vit_amd/csrc FFN=-DSMOE_FFN_FUSED` compiles it back in.
FFN_FUSED = _os.environ.get("SLIMMOE_FFN_FUSED", "0") == "1"


def ffn_fused_available() -> bool:
    return _lib.has_symbol("smoe_expert_ffn")
_ffn_ws = {}   # (device index, stream) -> the fused launch's kept-zero workspace


def _ffn_workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    """Ticket / row-counter words of smoe_expert_ffn: allocated ZEROED once per device and stream; every launch leaves them zero
    (the last workgroup to leave clears them), so no clearing launch runs in front of the GEMMs.  Keyed by the stream: launches on
    two streams may overlap and must not share counters."""
    key = (dev.index, _raw_stream(dev.index) if _raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream)
    t = _ffn_ws.get(key)
    if t is None or t.numel() < nbytes:
        t = _ffn_ws[key] = torch.zeros(max(nbytes, 1 << 14), dtype=torch.uint8, device=dev)
    return t


def ffn_workspace_error(dev: torch.device) -> bool:
    """True if any fused FFN launch on this device ever ran out of its wait on a row counter (reads the error words: a sync)."""
    return any(bool(t.view(torch.int32)[17].item()) for (d, _), t in _ffn_ws.items() if d == dev.index)   # FUSED_WS_ERR


def expert_ffn(X: torch.Tensor, W1: torch.Tensor, b1: Optional[torch.Tensor], W2: torch.Tensor, b2: Optional[torch.Tensor],
               offsets: torch.Tensor, out: torch.Tensor, a_gather: Optional[torch.Tensor] = None, a_div: int = 1,
               row_map: Optional[torch.Tensor] = None, row_scale: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, group_expert: Optional[torch.Tensor] = None,
               H: Optional[torch.Tensor] = None, rows_hint: Optional[int] = None) -> Optional[torch.Tensor]:
    """``out[row_map[r]] = residual[row_map[r]] + row_scale[row_map[r]] * (gelu(X[a_gather[r] / a_div] W1[e]^T + b1[e]) W2[e]^T + b2[e])``
    -- both expert GEMMs of a MoE layer with the top-1 combine -- in ONE persistent launch (smoe_expert_ffn); bit-identical to
    grouped_gemm(EPI_GELU) followed by grouped_gemm(row_map, row_scale, residual).  Returns ``out``, or None when the shape is
    outside the fused launch's reach (the caller then issues the two launches)."""
    _chk(X, "X", ndim=2)
    _chk(W1, "W1", X.dtype, 3)
    _chk(W2, "W2", X.dtype, 3)
    _chk(offsets, "offsets", torch.int32, 1)
    _chk(out, "out", torch.float32, 2)
    E, h, d_in = W1.shape
    E2, d_out, h2 = W2.shape
    if X.shape[1] != d_in or h2 != h or E2 != E or out.shape[1] != d_out:
        raise RuntimeError(f"expert_ffn: shapes disagree: X {tuple(X.shape)}, W1 {tuple(W1.shape)}, W2 {tuple(W2.shape)}, out {tuple(out.shape)}")
    M = X.shape[0]
    if a_gather is not None:
        _chk(a_gather, "a_gather", torch.int64, 1, align=8)
        M = a_gather.numel()
    G = offsets.numel() - 1
    if group_expert is None:
        if G != E:
            raise RuntimeError("offsets: expected E+1 entries")
    else:
        _chk(group_expert, "group_expert", torch.int32, 1)
    for t, nm, n in ((b1, "b1", h), (b2, "b2", d_out)):
        if t is not None:
            _chk(t, nm, torch.float32, 2)
            if tuple(t.shape) != (E, n):
                raise RuntimeError(f"{nm}: expected [E,{n}]")
    if row_map is not None:
        _chk(row_map, "row_map", torch.int64, 1, align=8)
    if row_scale is not None:
        _chk(row_scale, "row_scale", torch.float32, align=4)
    if residual is not None:
        _chk(residual, "residual", torch.float32, 2)
        if tuple(residual.shape) != tuple(out.shape):
            raise RuntimeError("residual: expected the shape of out")
    if X.dtype not in (torch.float16, torch.bfloat16) or M == 0:
        return None
    if a_gather is not None and X.numel() * X.element_size() >= 2 ** 32:
        return None     # 32-bit byte offsets into X, of which the library sees a_gather.numel() rows only: the two launches handle it
    if not ffn_fused_available():
        raise _lib.SlimMoEError("smoe_expert_ffn is not in this build of libslimmoe_hip.so (it measured slower than the two launches and "
                                "left the default build in round 5): make -C slim-switch-moe-vit_amd/csrc FFN=-DSMOE_FFN_FUSED")
    if H is None:
        H = torch.empty((M, h), dtype=X.dtype, device=X.device)
    else:
        _chk(H, "H", X.dtype, 2)
    lib = _lib.load()
    ws_bytes = lib.smoe_expert_ffn_workspace_bytes(M, G)
    ws = _ffn_workspace(X.device, ws_bytes)
    rows = M if rows_hint is None else rows_hint
    with _timed("expert_ffn", {"flops": 2.0 * rows * h * (d_in + d_out)}, X):
        rc = lib.smoe_expert_ffn(_ptr(X), _ptr(a_gather), a_div, _ptr(W1), _ptr(b1), _ptr(H), _ptr(W2), _ptr(b2), _ptr(offsets),
                                 _ptr(group_expert), G, E, M, d_in, h, d_out, dtype_code(X.dtype), _ptr(row_map), _ptr(row_scale),
                                 _ptr(residual), _ptr(out), out.shape[0], F32, _ptr(ws), ws.numel(), _stream(X))
    if rc == -1:
        return None
    _lib.check(rc, "smoe_expert_ffn")
    return out


def grouped_gemm_gelu_keep(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], offsets: torch.Tensor,
                           group_expert: Optional[torch.Tensor] = None, variant: int = DEFAULT_GEMM_VARIANT,
                           group_end: Optional[torch.Tensor] = None):
    """(H, gelu(H)) with H = A W[e]^T + bias[e] per row group -- the first expert linear of the training forward, which keeps
    both (gelu' needs H, the second linear's weight gradient needs gelu(H)): one epilogue with two stores where the kernel
    has it, else the GEMM followed by the GELU pass."""
    _chk(A, "A", ndim=2)
    _chk(W, "W", A.dtype, 3)
    _chk(offsets, "offsets", torch.int32, 1)
    M, K = A.shape
    E, N, _ = W.shape
    G = offsets.numel() - 1 if group_end is None else group_end.numel()
    if group_end is not None:
        _chk(group_end, "group_end", torch.int32, 1)
    if A.dtype in (torch.float16, torch.bfloat16) and W.shape[2] == K and (group_expert is not None or G == E):
        if bias is not None:
            _chk(bias, "bias", torch.float32, 2)
        if group_expert is not None:
            _chk(group_expert, "group_expert", torch.int32, 1)
        pre = torch.empty((M, N), dtype=A.dtype, device=A.device)
        out = torch.empty((M, N), dtype=A.dtype, device=A.device)
        rc = _lib.load().smoe_grouped_gemm_gelu_keep(_ptr(A), _ptr(W), _ptr(bias), _ptr(offsets), _ptr(group_expert), _ptr(group_end),
                                                     G, E, M, K, N, dtype_code(A.dtype), _ptr(pre), _ptr(out), _stream(A))
        if rc == 0:
            return pre, out
        if rc != -1:
            _lib.check(rc, "smoe_grouped_gemm_gelu_keep")
    if group_end is not None:
        raise RuntimeError("grouped_gemm_gelu_keep: separate row ranges (group_end) need the persistent kernel's shapes "
                           "(16-bit operands, K % 64 == 0, <= 63 groups)")
    pre = grouped_gemm(A, W, bias, offsets, EPI_NONE, A.dtype, variant=variant, group_expert=group_expert)
    return pre, gelu(pre)


def cast(src: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    _chk(src, "src")
    dst = torch.empty(src.shape, dtype=dtype, device=src.device)
    lib = _lib.load()
    rc = lib.smoe_cast(_ptr(src), dtype_code(src.dtype), _ptr(dst), dtype_code(dtype), src.numel(), _stream(src))
    _lib.check(rc, "smoe_cast")
    return dst


# ------------------------------------------------------------------------------------------ counter-based dropout
@functools.lru_cache(maxsize=64)
def dropout_params(p: float):
    """``(thr16, scale)`` of a drop probability: an element is kept iff its 16-bit draw is below ``thr16 = round((1 - p) * 65536)``
    (ties to even: p = 1 - 2^-17 keeps nothing) and kept values are multiplied by ``scale = f32(65536 / thr16)`` -- the inverse of
    the keep probability really applied, so the expectation is unbiased; 0 when nothing is kept."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    thr16 = min(65536, max(0, int(round((1.0 - p) * 65536.0))))
    scale = 65536.0 / thr16 if thr16 else 0.0
    return thr16, torch.tensor(scale, dtype=torch.float64).float().item()   # rounded once to f32, as the C call will pass it


def dropout_key(device) -> torch.Tensor:
    """A fresh mask key: int64 [2] = (k, c) on ``device``, ONE draw from torch's generator (``torch.manual_seed`` reproduces a run; a
    captured draw advances on every replay, as the captured ``randn`` / ``bernoulli_`` draws do).  The kernels read it from memory."""
    return torch.randint(-(1 << 63), (1 << 63) - 1, (2,), dtype=torch.int64, device=device)


def _drop_args(x: torch.Tensor, key: torch.Tensor, row_scale, name: str):
    _chk(x, name)
    _chk(key, "key", torch.int64, align=8)
    if key.numel() != 2:
        raise ValueError(f"dropout key: int64 [2], got {tuple(key.shape)}")
    if x.dim() < 1 or x.shape[-1] % 8 or x.shape[-1] == 0:
        raise ValueError(f"{name}: the last dimension must be a positive multiple of 8, got {tuple(x.shape)}")
    cols = x.shape[-1]
    rows = x.numel() // cols
    if row_scale is not None:
        _chk(row_scale, "row_scale", torch.float32, align=4)
        if row_scale.numel() != rows:
            raise ValueError(f"row_scale: {rows} rows expected, got {tuple(row_scale.shape)}")
    return rows, cols


def dropout(x: torch.Tensor, key: torch.Tensor, p: float, out_dtype: Optional[torch.dtype] = None, row_scale=None,
            out: Optional[torch.Tensor] = None, first_block: int = 0) -> torch.Tensor:
    """``select(kept, x * scale [* row_scale[row]], +0)`` in ``out_dtype`` (default: x's) with the mask of ``key`` (include/slimmoe.h:
    the rule).  Rows are the leading dimensions, the last dimension (a multiple of 8) the columns.  ``out=x`` runs in place.  The
    backward of a dropout IS this call on the gradient with the same key.  ``first_block``: the number of 8-element blocks in front
    of ``x`` when it is a row piece of a larger tensor."""
    rows, cols = _drop_args(x, key, row_scale, "x")
    thr16, scale = dropout_params(p)
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    else:
        _chk(out, "out", out_dtype)
        if out.shape != x.shape:
            raise ValueError(f"out: shape {tuple(x.shape)} expected, got {tuple(out.shape)}")
    rc = _lib.load().smoe_dropout(_ptr(x), _ptr(out), _ptr(row_scale), _ptr(key), int(first_block) & 0xFFFFFFFFFFFFFFFF, rows, cols,
                                  thr16, scale, dtype_code(x.dtype), dtype_code(out.dtype), _stream(x))
    _lib.check(rc, "smoe_dropout")
    return out


def dropout_add(h: torch.Tensor, residual: torch.Tensor, key: torch.Tensor, p: float, row_scale=None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``residual + select(kept, h * scale [* row_scale[row]], +0)``, f32: the attention half's tail ``x + drop_path(proj_drop(h))`` in
    one pass.  ``out=residual`` runs in place."""
    rows, cols = _drop_args(h, key, row_scale, "h")
    _chk(residual, "residual", torch.float32)
    if residual.shape != h.shape:
        raise ValueError(f"residual: shape {tuple(h.shape)} expected, got {tuple(residual.shape)}")
    thr16, scale = dropout_params(p)
    if out is None:
        out = torch.empty_like(residual)
    else:
        _chk(out, "out", torch.float32)
        if out.shape != h.shape:
            raise ValueError(f"out: shape {tuple(h.shape)} expected, got {tuple(out.shape)}")
    rc = _lib.load().smoe_dropout_add(_ptr(h), _ptr(residual), _ptr(row_scale), _ptr(out), _ptr(key), 0, rows, cols, thr16, scale,
                                      dtype_code(h.dtype), _stream(h))
    _lib.check(rc, "smoe_dropout_add")
    return out


def transpose_cast(src: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """``src [B, R, C] -> [B, C, R]`` in ``dtype`` (R, C multiples of 64): the second, transposed operand image of an expert
    weight that the dgrad GEMMs read, made in one pass from the master weight."""
    _chk(src, "src")
    if src.dim() != 3 or src.shape[1] % 64 or src.shape[2] % 64:
        raise ValueError(f"transpose_cast: [B, R, C] with R, C multiples of 64, got {tuple(src.shape)}")
    B, R, C = src.shape
    dst = torch.empty((B, C, R), dtype=dtype, device=src.device)
    rc = _lib.load().smoe_transpose_cast(_ptr(src), dtype_code(src.dtype), _ptr(dst), dtype_code(dtype), B, R, C, _stream(src))
    _lib.check(rc, "smoe_transpose_cast")
    return dst


# ------------------------------------------------------------------------------------------ backward pieces
def gelu(src: torch.Tensor) -> torch.Tensor:
    _chk(src, "src")
    dst = torch.empty_like(src)
    rc = _lib.load().smoe_gelu(_ptr(src), _ptr(dst), dtype_code(src.dtype), src.numel(), _stream(src))
    _lib.check(rc, "smoe_gelu")
    return dst


def rowdot(dout: torch.Tensor, y: torch.Tensor, inv_pos: torch.Tensor, k: int) -> torch.Tensor:
    """dscore[i] = <dout[i // k], y[inv_pos[i]]> (0 for dropped entries)."""
    _chk(dout, "dout", ndim=2)
    _chk(y, "y", ndim=2)
    _chk(inv_pos, "inv_pos", torch.int64, align=8)
    n = inv_pos.numel()
    out = torch.empty(n, dtype=torch.float32, device=dout.device)
    rc = _lib.load().smoe_rowdot(_ptr(dout), dtype_code(dout.dtype), _ptr(y), dtype_code(y.dtype), _ptr(inv_pos), n, k,
                                 dout.shape[1], _ptr(out), _stream(dout))
    _lib.check(rc, "smoe_rowdot")
    return out


def switch_aux(probs: torch.Tensor, counts: torch.Tensor):
    """(aux f32 [] , coef f32 [E]): the SwitchGate's load-balance loss E sum_e frac_e prob_e from the router's probabilities [T, E] and
    the plan's kept counts (i32 [E]), and d aux / d probs[t, e] = E frac_e / kept -- two launches, no host-launched [E]-sized ops."""
    _chk(probs, "probs", torch.float32, 2, align=4)
    _chk(counts, "counts", torch.int32, 1)
    T, E = probs.shape
    if counts.numel() != E:
        raise RuntimeError("switch_aux: one count per expert")
    lib = _lib.load()
    out = torch.empty(E + 1, dtype=torch.float32, device=probs.device)
    ws_bytes = lib.smoe_switch_aux_workspace_bytes(T, E)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=probs.device)
    rc = lib.smoe_switch_aux(_ptr(probs), _ptr(counts), T, E, _ptr(out), out.data_ptr() + 4, _ptr(ws), ws_bytes, _stream(probs))
    _lib.check(rc, "smoe_switch_aux")
    return out[0], out[1:]


def switch_gate_bwd(probs: torch.Tensor, idx: torch.Tensor, dscore: Optional[torch.Tensor], coef: Optional[torch.Tensor],
                    coef_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dlogits [T, E] of the SwitchGate's score (= probs[t, idx[t]]) and load-balance loss in one pass (softmax backward of
    g[t, e] = coef[e] * coef_scale + (e == idx[t]) dscore[t]); ``coef_scale``: a one-element f32 device tensor (d loss / d aux)."""
    _chk(probs, "probs", torch.float32, 2, align=4)
    T, E = probs.shape
    _chk(idx, "idx", torch.int64, align=8)
    if idx.numel() != T:
        raise RuntimeError("switch_gate_bwd: one index per token")
    if dscore is not None:
        _chk(dscore, "dscore", torch.float32, align=4)
    if coef is not None:
        _chk(coef, "coef", torch.float32, 1, align=4)
    if coef_scale is not None:
        _chk(coef_scale, "coef_scale", torch.float32, align=4)
    out = torch.empty_like(probs)
    rc = _lib.load().smoe_switch_gate_bwd(_ptr(probs), _ptr(idx), _ptr(dscore), _ptr(coef), _ptr(coef_scale), T, E, _ptr(out),
                                          _stream(probs))
    _lib.check(rc, "smoe_switch_gate_bwd")
    return out


def _gshard_pairs(t: torch.Tensor, name: str, dtype, T: Optional[int] = None) -> int:
    """``t`` is a contiguous [T, 2] tensor of ``dtype`` (the top-2 router's layout); returns T."""
    _chk(t, name, dtype, align=8 if dtype == torch.int64 else 4)
    if t.dim() != 2 or t.shape[1] != 2:
        raise RuntimeError(f"{name}: expected [T, 2] (the GShard gate is top-2), got {tuple(t.shape)}")
    if T is not None and t.shape[0] != T:
        raise RuntimeError(f"{name}: expected {T} rows, got {t.shape[0]}")
    return t.shape[0]


def gshard_prune(idx: torch.Tensor, score: torch.Tensor, u: Optional[torch.Tensor], E: int, capacity: int = -1):
    """(idx_out i64 [T, 2], top1_counts i32 [E]): the GShard gate's capacity and random routing on the top-2 router's ``idx`` /
    ``score`` [T, 2] (smoe_gshard_prune).  Entry 2 t + j is kept while fewer than ``capacity`` earlier flat entries named its expert
    (< 0: no clamp); then, with ``u`` (f32 [T]), a second choice with 2 score[t, 1] < u[t] is dropped.  Dropped entries are -1;
    top1_counts[e] counts the first choices before any drop.  Two launches."""
    T = _gshard_pairs(idx, "idx", torch.int64)
    _gshard_pairs(score, "score", torch.float32, T)
    if u is not None:
        _chk(u, "u", torch.float32, 1, align=4)
        if u.numel() != T:
            raise RuntimeError(f"u: expected {T} entries, got {u.numel()}")
    dev = idx.device
    lib = _lib.load()
    ws_bytes = lib.smoe_gshard_prune_workspace_bytes(T, int(E))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    idx_out = torch.empty_like(idx)
    top1 = torch.empty(int(E), dtype=torch.int32, device=dev)
    with _timed("gshard_prune", {"bytes": T * 44}, idx):
        rc = lib.smoe_gshard_prune(_ptr(idx), _ptr(score), _ptr(u), T, int(E), int(capacity), _ptr(idx_out), _ptr(top1), _ptr(ws),
                                   ws_bytes, _stream(idx))
    _lib.check(rc, "smoe_gshard_prune")
    return idx_out, top1


def gshard_aux(logits: torch.Tensor, top1_counts: torch.Tensor, num_expert: int):
    """(aux f32 [], coef f32 [E]): the GShard balance loss mean_e(c_e m_e) num_expert^2 from the router's logits [T, E] (row softmax in
    f32) and the first choices' counts (i32 [E]), and coef[e] = d aux / d softmax(logits)[t, e] -- two launches, bit-reproducible."""
    _chk(logits, "logits", torch.float32, 2, align=4)
    _chk(top1_counts, "top1_counts", torch.int32, 1, align=4)
    T, E = logits.shape
    if top1_counts.numel() != E:
        raise RuntimeError("gshard_aux: one count per expert")
    lib = _lib.load()
    out = torch.empty(E + 1, dtype=torch.float32, device=logits.device)
    ws_bytes = lib.smoe_gshard_aux_workspace_bytes(T, E)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=logits.device)
    with _timed("gshard_aux", {"bytes": 2 * T * E * 4}, logits):
        rc = lib.smoe_gshard_aux(_ptr(logits), _ptr(top1_counts), T, E, int(num_expert), _ptr(out), out.data_ptr() + 4, _ptr(ws), ws_bytes,
                                 _stream(logits))
    _lib.check(rc, "smoe_gshard_aux")
    return out[0], out[1:]


def gshard_gate_bwd(logits: torch.Tensor, idx: torch.Tensor, idx_out: torch.Tensor, score: torch.Tensor,
                    dscore: Optional[torch.Tensor], coef: Optional[torch.Tensor], coef_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dlogits [T, E] of the GShard gate's score (softmax over the two chosen logits; ``dscore`` [T, 2] counts only where ``idx_out`` >= 0)
    and balance loss (``coef`` from gshard_aux times ``coef_scale``, a one-element f32 device tensor = d loss / d aux) in one pass."""
    _chk(logits, "logits", torch.float32, 2, align=4)
    T, E = logits.shape
    _gshard_pairs(idx, "idx", torch.int64, T)
    _gshard_pairs(idx_out, "idx_out", torch.int64, T)
    _gshard_pairs(score, "score", torch.float32, T)
    if dscore is not None:
        _gshard_pairs(dscore, "dscore", torch.float32, T)
    if coef is not None:
        _chk(coef, "coef", torch.float32, 1, align=4)
        if coef.numel() != E:
            raise RuntimeError("gshard_gate_bwd: one coefficient per expert")
    if coef_scale is not None:
        _chk(coef_scale, "coef_scale", torch.float32, align=4)
        if coef is None or coef_scale.numel() != 1:
            raise RuntimeError("gshard_gate_bwd: coef_scale is one element and needs coef")
    out = torch.empty_like(logits)
    with _timed("gshard_gate_bwd", {"bytes": 2 * T * E * 4 + T * 56}, logits):
        rc = _lib.load().smoe_gshard_gate_bwd(_ptr(logits), _ptr(idx), _ptr(idx_out), _ptr(score), _ptr(dscore), _ptr(coef),
                                              _ptr(coef_scale), T, E, _ptr(out), _stream(logits))
    _lib.check(rc, "smoe_gshard_gate_bwd")
    return out


NOISY_MAX_E, NOISY_MAX_K = 32, 4     # the range of smoe_noisy_gate_fwd / _bwd (2 <= E, 1 <= k < E)


def noisy_gate_supported(E: int, k: int) -> bool:
    return 2 <= E <= NOISY_MAX_E and 1 <= k <= NOISY_MAX_K and k < E


def _noisy_logits2(logits2: torch.Tensor, eps: Optional[torch.Tensor]):
    """``logits2`` is a contiguous f32 [T, 2E] tensor ([clean | raw]) and ``eps`` f32 [T, E] or None; returns (T, E)."""
    _chk(logits2, "logits2", torch.float32, 2, align=4)
    T, E2 = logits2.shape
    if E2 % 2:
        raise RuntimeError(f"logits2: expected [T, 2E] (clean | raw), got {tuple(logits2.shape)}")
    if eps is not None:
        _chk(eps, "eps", torch.float32, 2, align=4)
        if tuple(eps.shape) != (T, E2 // 2):
            raise RuntimeError(f"eps: expected {(T, E2 // 2)}, got {tuple(eps.shape)}")
    return T, E2 // 2


def noisy_gate_fwd(logits2: torch.Tensor, eps: Optional[torch.Tensor], k: int, training: bool = True):
    """The noisy top-k gate's forward on the router's ``logits2`` [T, 2E] = [clean | raw] (smoe_noisy_gate_fwd; rule in INTEGRATION.md).
    Returns a dict: ``idx`` i64 [T, k], ``score`` f32 [T, k] (softmax over the k largest noisy values), ``keep`` f64 [T, 2] =
    (v_k, v_{k+1}) and ``next`` i32 [T] = the (k+1)-th expert (what noisy_gate_bwd wants kept), ``imp`` / ``load`` f32 [E], ``aux`` f32 []
    = cv2(imp) + cv2(load), ``coef_imp`` / ``coef_load`` f32 [E] = d aux / d imp, d aux / d load.  ``eps`` None = zero noise;
    ``training`` False = sigma 0 (no noise, no load term).  Two launches, bit-reproducible."""
    T, E = _noisy_logits2(logits2, eps)
    dev = logits2.device
    lib = _lib.load()
    ws_bytes = lib.smoe_noisy_gate_workspace_bytes(T, E)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    idx = torch.empty((T, int(k)), dtype=torch.int64, device=dev)
    score = torch.empty((T, int(k)), dtype=torch.float32, device=dev)
    keep = torch.empty((T, 2), dtype=torch.float64, device=dev)
    nxt = torch.empty((T,), dtype=torch.int32, device=dev)
    vec = torch.empty(4 * E + 1, dtype=torch.float32, device=dev)       # imp | load | coef_imp | coef_load | aux
    base = vec.data_ptr()
    with _timed("noisy_gate_fwd", {"bytes": T * (12 * E + 12 * int(k) + 20)}, logits2):
        rc = lib.smoe_noisy_gate_fwd(_ptr(logits2), _ptr(eps), T, E, int(k), 1 if training else 0, _ptr(idx), _ptr(score), _ptr(keep),
                                     _ptr(nxt), base, base + 4 * E, base + 16 * E, base + 8 * E, base + 12 * E, _ptr(ws), ws_bytes,
                                     _stream(logits2))
    _lib.check(rc, "smoe_noisy_gate_fwd")
    return dict(idx=idx, score=score, keep=keep, next=nxt, imp=vec[:E], load=vec[E:2 * E], coef_imp=vec[2 * E:3 * E],
                coef_load=vec[3 * E:4 * E], aux=vec[4 * E])


def noisy_gate_bwd(logits2: torch.Tensor, eps: Optional[torch.Tensor], idx: torch.Tensor, keep: torch.Tensor, nxt: torch.Tensor,
                   dscore: Optional[torch.Tensor], coef_imp: Optional[torch.Tensor],
                   coef_load: Optional[torch.Tensor], coef_scale: Optional[torch.Tensor] = None, training: bool = True) -> torch.Tensor:
    """dlogits2 [T, 2E] of the noisy gate's score (``dscore`` [T, k] or None) and loss (``coef_imp`` / ``coef_load`` from noisy_gate_fwd
    times ``coef_scale``, a one-element f32 device tensor = d loss / d aux; None = the loss is not in the objective) in one pass."""
    T, E = _noisy_logits2(logits2, eps)
    _chk(idx, "idx", torch.int64, 2, align=8)
    k = idx.shape[1]
    if idx.shape[0] != T:
        raise RuntimeError(f"idx: expected {T} rows, got {idx.shape[0]}")
    if dscore is not None:
        _chk(dscore, "dscore", torch.float32, 2, align=4)
        if tuple(dscore.shape) != (T, k):
            raise RuntimeError(f"dscore: expected {(T, k)}, got {tuple(dscore.shape)}")
    _chk(keep, "keep", torch.float64, 2, align=8)
    _chk(nxt, "next", torch.int32, 1, align=4)
    if tuple(keep.shape) != (T, 2) or nxt.numel() != T:
        raise RuntimeError("noisy_gate_bwd: keep is [T, 2] and next [T], as noisy_gate_fwd wrote them")
    if coef_scale is not None:
        _chk(coef_scale, "coef_scale", torch.float32, align=4)
        if coef_imp is None or coef_load is None or coef_scale.numel() != 1:
            raise RuntimeError("noisy_gate_bwd: coef_scale is one element and needs both coefficient vectors")
    for t, name in ((coef_imp, "coef_imp"), (coef_load, "coef_load")):
        if t is not None:
            _chk(t, name, torch.float32, 1, align=4)
            if t.numel() != E:
                raise RuntimeError(f"noisy_gate_bwd: {name} holds one coefficient per expert")
    out = torch.empty_like(logits2)
    with _timed("noisy_gate_bwd", {"bytes": T * (20 * E + 12 * k + 20)}, logits2):
        rc = _lib.load().smoe_noisy_gate_bwd(_ptr(logits2), _ptr(eps), _ptr(idx), _ptr(keep), _ptr(nxt), _ptr(dscore),
                                             _ptr(coef_imp), _ptr(coef_load), _ptr(coef_scale), T, E, k, 1 if training else 0, _ptr(out),
                                             _stream(logits2))
    _lib.check(rc, "smoe_noisy_gate_bwd")
    return out


def pad_offsets(offsets: torch.Tensor) -> torch.Tensor:
    _chk(offsets, "offsets", torch.int32, 1)
    out = torch.empty_like(offsets)
    rc = _lib.load().smoe_pad_offsets(_ptr(offsets), offsets.numel() - 1, _ptr(out), _stream(offsets))
    _lib.check(rc, "smoe_pad_offsets")
    return out


def split_offsets(offsets: torch.Tensor, S: int) -> torch.Tensor:
    """i32 [G * S + 1]: every row group of ``offsets`` cut into S pseudo-groups of whole 64-row chunks (smoe_split_offsets)."""
    _chk(offsets, "offsets", torch.int32, 1, align=4)
    G = offsets.numel() - 1
    out = torch.empty(G * int(S) + 1, dtype=torch.int32, device=offsets.device)
    rc = _lib.load().smoe_split_offsets(_ptr(offsets), G, int(S), _ptr(out), _stream(offsets))
    _lib.check(rc, "smoe_split_offsets")
    return out


def expert_wgrad_splits(G: int, R1: int, R2: int, rows: int, device) -> int:
    """Pieces to cut every expert's rows into for its weight gradient [R1, R2]: the kernel's grid is groups x output tiles, and at
    small widths that is a fraction of the chip (DeiT-Tiny, models/resMoE.py:151-187: 8 experts x 3 tiles = 24 workgroups walking 6 k rows
    each, 100 us per launch and a third of the training step).  Enough pieces for ~one round of workgroups, at least ~512 rows each."""
    tiles = G * min(-(-R1 // 256) * -(-R2 // 256), -(-R2 // 256) * -(-R1 // 256))
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    if tiles * 2 > cus:
        return 1
    return max(1, min(16, cus // max(tiles, 1), rows // max(G, 1) // 512))


def split_ranges(starts: torch.Tensor, ends: torch.Tensor, S: int):
    """smoe_split_offsets' rule for SEPARATE row ranges [starts[g], ends[g]) (the slots of the static expert exchange): S pieces of whole
    64-row chunks each, the last ones possibly empty -> (starts i32 [G * S], ends i32 [G * S]); a few [G, S]-sized device ops, no sync."""
    cnt = (ends - starts).to(torch.int64).view(-1, 1)
    step = ((cnt + S * 64 - 1) // (S * 64)) * 64
    at = torch.arange(S, device=starts.device, dtype=torch.int64).view(1, S) * step
    lo = starts.to(torch.int64).view(-1, 1)
    s0 = lo + torch.minimum(at, cnt)
    e0 = lo + torch.minimum(at + step, cnt)
    return s0.reshape(-1).to(torch.int32).contiguous(), e0.reshape(-1).to(torch.int32).contiguous()


def grouped_wgrad_rows_split(P: torch.Tensor, Q: torch.Tensor, offsets: torch.Tensor, S: int,
                             offsets_split=None, group_end: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``grouped_wgrad_rows`` with every group cut into S pieces (``offsets_split`` = split_offsets(offsets, S), reusable by the
    layer's second weight gradient) and the partial products summed in piece order: f32 [G, R1, R2].  With ``group_end`` (separate
    row ranges) ``offsets_split`` is the pair split_ranges(offsets, group_end, S)."""
    if group_end is not None:
        G = group_end.numel()
        if S <= 1:
            return grouped_wgrad_rows(P, Q, offsets, group_end=group_end)
        s0, e0 = offsets_split if offsets_split is not None else split_ranges(offsets, group_end, S)
        part = grouped_wgrad_rows(P, Q, s0, group_end=e0)
        return part.view(G, S, part.shape[1], part.shape[2]).sum(1)
    G = offsets.numel() - 1
    if S <= 1:
        return grouped_wgrad_rows(P, Q, offsets)
    if offsets_split is None:
        offsets_split = split_offsets(offsets, S)
    part = grouped_wgrad_rows(P, Q, offsets_split)
    return part.view(G, S, part.shape[1], part.shape[2]).sum(1)


def padded_len(n_rows: int, E: int) -> int:
    """Static upper bound of offsets_pad[E]: every expert range rounded up to 64."""
    return ((n_rows + 63) // 64) * 64 + 64 * E


def transpose_pad(src: torch.Tensor, offsets: torch.Tensor, offsets_pad: torch.Tensor, Lp: int) -> torch.Tensor:
    """[n, C] expert-sorted rows -> [C, Lp] K-major image with 64-aligned, zero-padded expert ranges."""
    _chk(src, "src", ndim=2)
    n, C = src.shape
    dst = torch.empty((C, Lp), dtype=src.dtype, device=src.device)
    rc = _lib.load().smoe_transpose_pad(_ptr(src), dtype_code(src.dtype), _ptr(offsets), _ptr(offsets_pad),
                                        offsets.numel() - 1, n, C, Lp, _ptr(dst), _stream(src))
    _lib.check(rc, "smoe_transpose_pad")
    return dst


def grouped_wgrad(PT: torch.Tensor, QT: torch.Tensor, offsets_pad: torch.Tensor) -> torch.Tensor:
    """out[e] = PT[:, range e] @ QT[:, range e]^T, f32 [E, R1, R2]."""
    _chk(PT, "PT", ndim=2)
    _chk(QT, "QT", PT.dtype, 2)
    E = offsets_pad.numel() - 1
    R1, Lp = PT.shape
    R2 = QT.shape[0]
    if QT.shape[1] != Lp:
        raise RuntimeError("PT / QT: padded lengths differ")
    out = torch.empty((E, R1, R2), dtype=torch.float32, device=PT.device)
    with _timed("grouped_wgrad", {"K": Lp}, PT):
        rc = _lib.load().smoe_grouped_wgrad(_ptr(PT), _ptr(QT), dtype_code(PT.dtype), _ptr(offsets_pad), E, R1, R2, Lp,
                                            _ptr(out), _stream(PT))
    _lib.check(rc, "smoe_grouped_wgrad")
    return out


_zero_pages = StreamCache()


_ones_cache = {}


def ones_f32(n: int, device) -> torch.Tensor:
    """A cached f32 vector of ones (read-only: unit combine weights of the scatter's adjoint) -- not a fill kernel per backward."""
    key = (torch.device(device).index, int(n))
    t = _ones_cache.get(key)
    if t is None:
        if len(_ones_cache) > 64:
            _ones_cache.clear()
        t = _ones_cache[key] = torch.ones(int(n), dtype=torch.float32, device=device)
    return t


def _zero16(device) -> torch.Tensor:
    return _zero_pages.get(str(device), 0, lambda: torch.zeros(64, dtype=torch.uint8, device=device))


def _wgrad_rounds(E: int, R1: int, R2: int, cus: int) -> float:
    """Cost-weighted rounds of workgroups of smoe_grouped_wgrad_rows (256- or 320-row tiles; csrc/gemm.hip launch_wgrad_rows)."""
    tn = -(-R2 // 256)
    c4 = -(-(E * -(-R1 // 256) * tn) // cus)
    c5 = 1.25 * -(-(E * -(-R1 // 320) * tn) // cus)
    return min(c4, c5)


def grouped_wgrad_rows(P: torch.Tensor, Q: torch.Tensor, offsets: torch.Tensor, allow_swap: bool = True,
                       group_end: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[e] (f32 [R1, R2]) = P[rows of e]^T @ Q[rows of e] from the token-major operands (no transposed copies).
    ``group_end`` (i32 [G]): separate row ranges [offsets[g], group_end[g]) (``offsets`` then needs G entries only).
    The kernel's tile is taller (256 / 320 output rows) than wide along R1 only, so when the transposed problem needs fewer
    rounds of workgroups (ViT-B's dW2 [768, 3072]: 288 tiles = two rounds on 256 CUs; as [3072, 768]: 240 taller tiles = one)
    it is computed as Q^T P and transposed back by smoe_transpose_cast (one pass over the f32 result)."""
    _chk(P, "P", ndim=2)
    _chk(Q, "Q", ndim=2)
    if P.dtype != Q.dtype or P.dtype not in (torch.float16, torch.bfloat16) or P.shape[0] != Q.shape[0]:
        raise RuntimeError("grouped_wgrad_rows: P and Q must be f16 / bf16 with the same row count")
    _chk(offsets, "offsets", torch.int32, 1)
    if group_end is not None:
        _chk(group_end, "group_end", torch.int32, 1)
        if offsets.numel() < group_end.numel() or P.numel() >= 2 ** 32 or Q.numel() >= 2 ** 32:
            raise RuntimeError("grouped_wgrad_rows: group_end needs an offsets entry per group and operands under 2^32 elements")
    E = offsets.numel() - 1 if group_end is None else group_end.numel()
    R1, R2 = P.shape[1], Q.shape[1]
    if P.numel() >= 2 ** 32 or Q.numel() >= 2 ** 32:
        # the token-major kernel addresses its operands with 32-bit ELEMENT offsets (csrc/gemm.hip MODE 2): an operand of
        # 2^32 elements or more takes the K-major path (64-padded transposed images, 64-bit row bases).  That path ends at
        # smoe_transpose_pad's own limit of 4,194,240 padded rows (its grid's second dimension): operands of 1,024 columns or fewer
        # have more rows than that by the time they hold 2^32 elements, and get its error instead of a result.
        offs_pad = pad_offsets(offsets)
        Lp = padded_len(P.shape[0], E)
        return grouped_wgrad(transpose_pad(P, offsets, offs_pad, Lp), transpose_pad(Q, offsets, offs_pad, Lp), offs_pad)
    if allow_swap and R1 % 64 == 0 and R2 % 64 == 0:
        cus = torch.cuda.get_device_properties(P.device).multi_processor_count
        if _wgrad_rounds(E, R2, R1, cus) + 0.15 < _wgrad_rounds(E, R1, R2, cus):
            return transpose_cast(grouped_wgrad_rows(Q, P, offsets, allow_swap=False, group_end=group_end), torch.float32)
    out = torch.empty((E, R1, R2), dtype=torch.float32, device=P.device)
    rc = _lib.load().smoe_grouped_wgrad_rows(_ptr(P), _ptr(Q), dtype_code(P.dtype), _ptr(offsets), _ptr(group_end), E, R1, R2,
                                              _ptr(_zero16(P.device)), _ptr(out), _stream(P))
    _lib.check(rc, "smoe_grouped_wgrad_rows")
    return out


def gate_wgrad(dl: torch.Tensor, x: torch.Tensor, want_bias: bool = False):
    """dWg [E, d] f32 = dl^T x for dl [T, E] f32, x [T, d]: the router weight gradient as a streaming reduction.
    ``want_bias``: returns (dWg, dbg [E] = column sums of dl) from the same pass."""
    _chk(dl, "dl", torch.float32, 2, align=4)
    _chk(x, "x", ndim=2)
    T, E = dl.shape
    C = x.shape[1]
    if x.shape[0] != T:
        raise RuntimeError("gate_wgrad: row counts differ")
    lib = _lib.load()
    out = torch.empty((E, C), dtype=torch.float32, device=x.device)
    db = torch.empty(E, dtype=torch.float32, device=x.device) if want_bias else None
    ws_bytes = lib.smoe_gate_wgrad_workspace_bytes(T, E, C)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    rc = lib.smoe_gate_wgrad(_ptr(dl), _ptr(x), dtype_code(x.dtype), T, E, C, _ptr(out), _ptr(db), _ptr(ws), ws_bytes, _stream(x))
    _lib.check(rc, "smoe_gate_wgrad")
    return (out, db) if want_bias else out


def gate_dgrad(dl: torch.Tensor, w: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """dx [T, d] = dl [T, E] @ w [E, d] (f32 inputs): the router linear's input gradient as a streaming kernel."""
    _chk(dl, "dl", torch.float32, 2, align=4)
    _chk(w, "w", torch.float32, 2)
    T, E = dl.shape
    if w.shape[0] != E:
        raise RuntimeError("gate_dgrad: dl / w disagree on E")
    d = w.shape[1]
    out = torch.empty((T, d), dtype=out_dtype, device=dl.device)
    rc = _lib.load().smoe_gate_dgrad(_ptr(dl), _ptr(w), T, E, d, _ptr(out), dtype_code(out_dtype), _stream(dl))
    _lib.check(rc, "smoe_gate_dgrad")
    return out


def zero_group_fold(cs2: torch.Tensor, cs1: Optional[torch.Tensor], A: torch.Tensor, offsets: torch.Tensor, gmap: torch.Tensor,
                    E: int, dW2: torch.Tensor, want_b2: bool = True, want_b1: bool = True):
    """The zero-row groups' share of the expert gradients in one launch (smoe_zero_group_fold): ``dW2`` [E, d, h] gets the rank-1
    terms colsum(dY_g) (x) A_row IN PLACE; returns (db2 [E, d] | None, db1 [E, h] | None) = own group's column sums + those of the
    zero groups mapped to the expert.  cs2 [G, d] / cs1 [G, h]: column sums over all G = E + Z groups."""
    _chk(cs2, "cs2", torch.float32, 2)
    _chk(A, "A", ndim=2)
    _chk(offsets, "offsets", torch.int32, 1, align=4)
    _chk(gmap, "gmap", torch.int32, 1, align=4)
    _chk(dW2, "dW2", torch.float32, 3)
    G, d = cs2.shape
    h = A.shape[1]
    Z = G - E
    if Z < 0 or offsets.numel() != G + 1 or gmap.numel() != G or tuple(dW2.shape) != (E, d, h) or h % 4:
        raise RuntimeError("zero_group_fold: shapes disagree")
    if cs1 is not None:
        _chk(cs1, "cs1", torch.float32, 2)
        if tuple(cs1.shape) != (G, h):
            raise RuntimeError("zero_group_fold: cs1 must be [G, h]")
    want_b1 = want_b1 and cs1 is not None
    db2 = torch.empty((E, d), dtype=torch.float32, device=cs2.device) if want_b2 else None
    db1 = torch.empty((E, h), dtype=torch.float32, device=cs2.device) if want_b1 else None
    rc = _lib.load().smoe_zero_group_fold(_ptr(cs2), _ptr(cs1), _ptr(A), dtype_code(A.dtype), _ptr(offsets), _ptr(gmap), E, Z, d, h,
                                          A.shape[0], _ptr(dW2), _ptr(db2), _ptr(db1), _stream(cs2))
    _lib.check(rc, "smoe_zero_group_fold")
    return db2, db1


def group_colsum(src: torch.Tensor, offsets: torch.Tensor, group_end: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[e, c] = sum of the rows of group e (bias gradients); deterministic two-pass reduction.  ``group_end`` (i32 [G]): separate
    row ranges [offsets[g], group_end[g]) -- ``offsets`` then needs G entries only."""
    _chk(src, "src", ndim=2)
    _chk(offsets, "offsets", torch.int32, 1)
    if group_end is not None:
        _chk(group_end, "group_end", torch.int32, 1)
        if offsets.numel() < group_end.numel():
            raise RuntimeError("group_colsum: offsets must have an entry per group")
    E = offsets.numel() - 1 if group_end is None else group_end.numel()
    n, C = src.shape
    lib = _lib.load()
    out = torch.empty((E, C), dtype=torch.float32, device=src.device)
    ws_bytes = lib.smoe_group_colsum_workspace_bytes(n, E, C)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=src.device)
    rc = lib.smoe_group_colsum(_ptr(src), dtype_code(src.dtype), _ptr(offsets), _ptr(group_end), E, n, C, _ptr(out), _ptr(ws),
                               ws_bytes, _stream(src))
    _lib.check(rc, "smoe_group_colsum")
    return out


# ------------------------------------------------------------------------------------------ Mixup / CutMix and the soft-target loss
def mixup_images_(x: torch.Tensor, lam: torch.Tensor, one_minus: torch.Tensor, box: torch.Tensor) -> torch.Tensor:
    """Mixup / CutMix of ``x`` f32 [B, C, H, W] IN PLACE (smoe_mixup_images): sample b with sample B-1-b, ``lam`` / ``one_minus`` f32 [B],
    ``box`` i32 [B, 4] = (yl, yh, xl, xh) per sample (empty = Mixup, non-empty = CutMix, lam == 1 = untouched).  B even."""
    _chk(x, "x", torch.float32, 4, align=4)
    B, C, H, W = x.shape
    _chk(lam, "lam", torch.float32, 1, align=4)
    _chk(one_minus, "one_minus", torch.float32, 1, align=4)
    _chk(box, "box", torch.int32, 2, align=4)
    if lam.numel() != B or one_minus.numel() != B or tuple(box.shape) != (B, 4):
        raise RuntimeError("mixup_images_: lam / one_minus [B] and box [B, 4] expected")
    rc = _lib.load().smoe_mixup_images(_ptr(x), B, C, H, W, _ptr(lam), _ptr(one_minus), _ptr(box), _stream(x))
    _lib.check(rc, "smoe_mixup_images")
    return x


def mixup_target(labels: torch.Tensor, lam: torch.Tensor, one_minus: torch.Tensor, on: float, off: float, num_classes: int) -> torch.Tensor:
    """f32 [B, num_classes] = one_hot(labels, on, off) * lam + one_hot(labels.flip(0), on, off) * one_minus (smoe_mixup_target)."""
    _chk(labels, "labels", torch.int64, 1, align=8)
    _chk(lam, "lam", torch.float32, 1, align=4)
    _chk(one_minus, "one_minus", torch.float32, 1, align=4)
    B = labels.numel()
    if lam.numel() != B or one_minus.numel() != B:
        raise RuntimeError("mixup_target: lam / one_minus [B] expected")
    out = torch.empty((B, int(num_classes)), dtype=torch.float32, device=labels.device)
    rc = _lib.load().smoe_mixup_target(_ptr(labels), _ptr(lam), _ptr(one_minus), float(on), float(off), B, int(num_classes), _ptr(out),
                                       _stream(labels))
    _lib.check(rc, "smoe_mixup_target")
    return out


def _soft_ce_args(logits, target, labels):
    _chk(logits, "logits", ndim=2, align=2)
    B, C = logits.shape
    if (target is None) == (labels is None):
        raise RuntimeError("soft_ce: exactly one of target (f32 [B, C]) and labels (i64 [B]) expected")
    if target is not None:
        _chk(target, "target", torch.float32, 2, align=4)
        if tuple(target.shape) != (B, C) or target.device != logits.device:
            raise RuntimeError("soft_ce: target must be f32 [B, C] on the logits' device")
    else:
        _chk(labels, "labels", torch.int64, 1, align=8)
        if labels.numel() != B or labels.device != logits.device:
            raise RuntimeError("soft_ce: labels must be i64 [B] on the logits' device")
    return B, C


def soft_ce_fwd(logits: torch.Tensor, target: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                smoothing: float = 0.0):
    """Mean over rows of sum(-t log_softmax(x)) (dense ``target``) or of the label-smoothing loss (``labels`` + ``smoothing``):
    (loss f32 [], rows f32 [4, B] = per-row loss, maximum, log of the sum of exp(x - max), target sum -- the last three are what
    soft_ce_bwd needs)."""
    B, C = _soft_ce_args(logits, target, labels)
    rows = torch.empty((4, B), dtype=torch.float32, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    rc = _lib.load().smoe_soft_ce_fwd(_ptr(logits), dtype_code(logits.dtype), _ptr(target), _ptr(labels), float(smoothing), B, C,
                                      _ptr(rows), rows.data_ptr() + 4 * B, rows.data_ptr() + 8 * B, rows.data_ptr() + 12 * B, _ptr(loss),
                                      _stream(logits))
    _lib.check(rc, "smoe_soft_ce_fwd")
    return loss, rows


def soft_ce_bwd(logits: torch.Tensor, rows: torch.Tensor, g: torch.Tensor, target: Optional[torch.Tensor] = None,
                labels: Optional[torch.Tensor] = None, smoothing: float = 0.0) -> torch.Tensor:
    """dlogits = g (softmax(x) sum(t) - t) / B in the logits' dtype; ``g``: device f32 scalar; ``rows``: soft_ce_fwd's."""
    B, C = _soft_ce_args(logits, target, labels)
    _chk(rows, "rows", torch.float32, 2, align=4)
    _chk(g, "g", torch.float32, align=4)
    if tuple(rows.shape) != (4, B) or g.numel() != 1 or g.device != logits.device:
        raise RuntimeError("soft_ce_bwd: rows f32 [4, B] and a device f32 scalar g expected")
    out = torch.empty_like(logits)
    rc = _lib.load().smoe_soft_ce_bwd(_ptr(logits), dtype_code(logits.dtype), _ptr(target), _ptr(labels), float(smoothing), B, C,
                                      rows.data_ptr() + 4 * B, rows.data_ptr() + 8 * B, rows.data_ptr() + 12 * B, _ptr(g), _ptr(out),
                                      _stream(logits))
    _lib.check(rc, "smoe_soft_ce_bwd")
    return out


# --------------------------------------------------------------------------------------------------------------- evaluation metrics
_topk_arrays = {}     # topk tuple -> the host int array smoe_eval_metrics reads (built once per tuple)


def eval_metrics(logits: torch.Tensor, labels: torch.Tensor, acc: Optional[torch.Tensor] = None, topk=(1, 5)):
    """Cross-entropy and top-k accuracy of a batch in two launches (smoe_eval_metrics): ``logits`` f32 / f16 / bf16 [B, C], ``labels``
    i64 [B], ``topk`` one to four k >= 1.  -> (batch f32 [1 + nk] = mean loss and the accuracies in percent, row_loss f32 [B], row_rank
    i32 [B] = the classes that come before the label's in a stable descending order, NaN largest, ties to the lower index).  ``acc``
    (optional): an f64 [2 + nk] accumulator on the logits' device, += (sum of the row losses, B, correct counts) -- no host read; use
    one accumulator from one stream at a time."""
    _chk(logits, "logits", ndim=2, align=2)
    B, C = logits.shape
    _chk(labels, "labels", torch.int64, 1, align=8)
    if labels.numel() != B or labels.device != logits.device:
        raise RuntimeError("eval_metrics: labels must be i64 [B] on the logits' device")
    ks = tuple(int(k) for k in topk)
    if not 1 <= len(ks) <= 4 or min(ks) < 1:
        raise RuntimeError(f"eval_metrics: topk must hold one to four k >= 1, not {topk!r}")
    if C < 1:
        raise RuntimeError("eval_metrics: logits [B, C] with C >= 1 expected")
    nk = len(ks)
    if acc is not None:
        _chk(acc, "acc", torch.float64, 1, align=8)
        if acc.numel() != 2 + nk or acc.device != logits.device:
            raise RuntimeError(f"eval_metrics: acc must be f64 [{2 + nk}] on the logits' device")
    dev = logits.device
    code = dtype_code(logits.dtype)
    row_loss = torch.empty(B, dtype=torch.float32, device=dev)
    row_rank = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:       # (the library returns at once: the mean of no rows is NaN, as torch's is)
        return torch.full((1 + nk,), float("nan"), dtype=torch.float32, device=dev), row_loss, row_rank
    batch = torch.empty(1 + nk, dtype=torch.float32, device=dev)
    karr = _topk_arrays.get(ks)
    if karr is None:
        karr = _topk_arrays[ks] = (ctypes.c_int * nk)(*ks)
    rc = _lib.load().smoe_eval_metrics(_ptr(logits), code, _ptr(labels), B, C, karr, nk, _ptr(row_loss), _ptr(row_rank), _ptr(batch),
                                       _ptr(acc), _stream(logits))
    _lib.check(rc, "smoe_eval_metrics")
    return batch, row_loss, row_rank


# ------------------------------------------------------------------------------------------------------------ knowledge distillation
DISTILL_SOFT, DISTILL_HARD = 0, 1
_DISTILL_MODES = {"soft": DISTILL_SOFT, "hard": DISTILL_HARD}


def _distill_args(student, teacher, mode):
    _chk(student, "student", ndim=2, align=2)
    _chk(teacher, "teacher", ndim=2, align=2)
    if mode not in _DISTILL_MODES:
        raise RuntimeError(f"distill: mode must be 'soft' or 'hard', not {mode!r}")
    if teacher.shape != student.shape or teacher.device != student.device:
        raise RuntimeError("distill: student and teacher logits must be [B, C] on one device")
    dtype_code(student.dtype), dtype_code(teacher.dtype)
    return student.shape[0], student.shape[1], _DISTILL_MODES[mode]


def distill_fwd(student: torch.Tensor, teacher: torch.Tensor, base_loss: torch.Tensor, mode: str, tau: float, alpha: float):
    """losses.py:53-72 on the device (smoe_distill_fwd): ``student`` (the distillation head's logits) and ``teacher`` [B, C], each f32 /
    f16 / bf16; ``base_loss`` a device f32 scalar.  -> (loss f32 [] = base (1 - alpha) + distill alpha, distill f32 [], row values
    f64 [B], stats f64 [4, B], labels i32 [B]); the last two are what distill_bwd needs."""
    B, C, m = _distill_args(student, teacher, mode)
    _chk(base_loss, "base_loss", torch.float32, align=4)
    if base_loss.numel() != 1 or base_loss.device != student.device:
        raise RuntimeError("distill_fwd: base_loss must be a device f32 scalar")
    dev = student.device
    rows = torch.empty(B, dtype=torch.float64, device=dev)
    stats = torch.empty((4, B), dtype=torch.float64, device=dev)
    labels = torch.empty(B, dtype=torch.int32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)            # (distill, loss)
    rc = _lib.load().smoe_distill_fwd(_ptr(student), dtype_code(student.dtype), _ptr(teacher), dtype_code(teacher.dtype), m, float(tau),
                                      float(alpha), _ptr(base_loss), B, C, _ptr(rows), _ptr(stats), _ptr(labels), _ptr(out),
                                      out.data_ptr() + 4, _stream(student))
    _lib.check(rc, "smoe_distill_fwd")
    return out[1], out[0], rows, stats, labels


def distill_bwd(student: torch.Tensor, teacher: torch.Tensor, stats: torch.Tensor, labels: torch.Tensor, g: torch.Tensor, mode: str,
                tau: float, alpha: float) -> torch.Tensor:
    """d loss / d student in the student's dtype (smoe_distill_bwd); ``g``: device f32 scalar; ``stats`` / ``labels``: distill_fwd's."""
    B, C, m = _distill_args(student, teacher, mode)
    _chk(stats, "stats", torch.float64, 2, align=8)
    _chk(labels, "labels", torch.int32, 1, align=4)
    _chk(g, "g", torch.float32, align=4)
    if tuple(stats.shape) != (4, B) or labels.numel() != B or g.numel() != 1 or g.device != student.device:
        raise RuntimeError("distill_bwd: stats f64 [4, B], labels i32 [B] and a device f32 scalar g expected")
    out = torch.empty_like(student)
    rc = _lib.load().smoe_distill_bwd(_ptr(student), dtype_code(student.dtype), _ptr(teacher), dtype_code(teacher.dtype), m, float(tau),
                                      float(alpha), B, C, _ptr(stats), _ptr(labels), _ptr(g), _ptr(out), _stream(student))
    _lib.check(rc, "smoe_distill_bwd")
    return out


# ------------------------------------------------------------------------------------------------- binary cross-entropy with logits
def _bce_args(logits, target):
    _chk(logits, "logits", ndim=2, align=2)
    dtype_code(logits.dtype)
    _chk(target, "target", torch.float32, 2, align=4)
    if target.shape != logits.shape or target.device != logits.device:
        raise RuntimeError("bce: target must be f32 [B, C] on the logits' device")
    return logits.shape[0], logits.shape[1]


def bce_fwd(logits: torch.Tensor, target: torch.Tensor, binarize: bool = False):
    """``torch.nn.BCEWithLogitsLoss()`` (reduction 'mean') on the device in two launches (smoe_bce_fwd): ``logits`` f32 / f16 / bf16
    [B, C], ``target`` f32 [B, C]; ``binarize``: every target counts as ``target > 0`` (engine.py:49-50).  -> (loss f32 [], row_loss
    f32 [B] = each row's sum of element losses)."""
    B, C = _bce_args(logits, target)
    row_loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    with _timed("bce_fwd", {"bytes": B * C * (logits.element_size() + 4)}, logits):
        rc = _lib.load().smoe_bce_fwd(_ptr(logits), dtype_code(logits.dtype), _ptr(target), int(bool(binarize)), B, C, _ptr(row_loss),
                                      _ptr(loss), _stream(logits))
    _lib.check(rc, "smoe_bce_fwd")
    return loss, row_loss


def bce_bwd(logits: torch.Tensor, target: torch.Tensor, g: torch.Tensor, binarize: bool = False) -> torch.Tensor:
    """dlogits = g (sigmoid(x) - t) / (B C) in the logits' dtype (smoe_bce_bwd); ``g``: device f32 scalar."""
    B, C = _bce_args(logits, target)
    _chk(g, "g", torch.float32, align=4)
    if g.numel() != 1 or g.device != logits.device:
        raise RuntimeError("bce_bwd: a device f32 scalar g expected")
    out = torch.empty_like(logits)
    with _timed("bce_bwd", {"bytes": B * C * (2 * logits.element_size() + 4)}, logits):
        rc = _lib.load().smoe_bce_bwd(_ptr(logits), dtype_code(logits.dtype), _ptr(target), int(bool(binarize)), B, C, _ptr(g), _ptr(out),
                                      _stream(logits))
    _lib.check(rc, "smoe_bce_bwd")
    return out


# ------------------------------------------------------------------------------------------------- SwitchableLayerNorm
SWITCH_LN_MAX_BUCKETS = 32


def switch_ln_supported(d: int, K: int) -> bool:
    """The reach of smoe_switch_ln_fwd / _bwd: d % 4 == 0, 4 <= d <= 1024 (LN_DIMS among them), 1 <= K <= 32 buckets."""
    return bool(_lib.load().smoe_switch_ln_supported(int(d), int(K)))


def _switch_ln_tables(x, weights, biases, centroids):
    d = x.shape[-1]
    K = None
    for t, name in ((weights, "weights"), (biases, "biases"), (centroids, "centroids")):
        if t is None:
            continue
        _chk(t, name, torch.float32, 2)
        if t.shape[1] != d or t.device != x.device or (K is not None and t.shape[0] != K):
            raise RuntimeError(f"switch_ln: {name} must be f32 [K, {d}] on x's device, got {tuple(t.shape)}")
        K = t.shape[0]
    return K


def switch_ln(x: torch.Tensor, weights: Optional[torch.Tensor], biases: Optional[torch.Tensor], centroids: Optional[torch.Tensor],
              eps: float, buckets=None, num_buckets: Optional[int] = None):
    """SwitchableLayerNorm's rule (models/layers.py:105-151) in one launch (smoe_switch_ln_fwd): ``x`` f32 [..., d]; ``weights`` /
    ``biases`` / ``centroids`` f32 [K, d] (weights and biases None: no affine); ``buckets``: None = selected per row (the exact argmin
    of the squared distances to the centroids; K == 1 reads no centroids), an int = that bucket for every row, or an int64 tensor
    of ``x.shape[:-1]``.  -> (y f32 like x, buckets int64 ``x.shape[:-1]``).  x is not modified."""
    _chk(x, "x", torch.float32)
    d = x.shape[-1]
    T = x.numel() // d if d else 0
    K = _switch_ln_tables(x, weights, biases, centroids)
    if K is None:
        K = num_buckets
    if K is None:
        raise RuntimeError("switch_ln: without tables the number of buckets must be given")
    if biases is not None and weights is None:
        raise RuntimeError("switch_ln: biases without weights")
    if not switch_ln_supported(d, K):
        raise RuntimeError(f"switch_ln: d={d}, K={K} outside the kernel's reach (d % 4 == 0, d <= 1024, K <= {SWITCH_LN_MAX_BUCKETS})")
    b_in, b_all = None, -1
    if isinstance(buckets, torch.Tensor):
        _chk(buckets, "buckets", torch.int64, align=8)
        if tuple(buckets.shape) != tuple(x.shape[:-1]) or buckets.device != x.device:
            raise RuntimeError("switch_ln: buckets must be int64 of x.shape[:-1] on x's device")
        b_in = buckets
    elif buckets is not None:
        b_all = int(buckets)
        if not 0 <= b_all < K:
            raise RuntimeError(f"switch_ln: bucket {b_all} outside [0, {K})")
    elif K > 1 and centroids is None:
        raise RuntimeError("switch_ln: centroids needed to select among K > 1 buckets")
    y = torch.empty_like(x)
    out_b = torch.empty(x.shape[:-1], dtype=torch.int64, device=x.device)
    with _timed("switch_ln", {"bytes": T * d * 8}, x):
        rc = _lib.load().smoe_switch_ln_fwd(_ptr(x), _ptr(weights), _ptr(biases), _ptr(centroids), _ptr(b_in), b_all, float(eps), T, d, K,
                                            _ptr(y), _ptr(out_b), _stream(x))
    _lib.check(rc, "smoe_switch_ln_fwd")
    return y, out_b


def switch_ln_bwd(x: torch.Tensor, dy: torch.Tensor, weights: Optional[torch.Tensor], buckets: torch.Tensor, eps: float,
                  num_buckets: Optional[int] = None, want_param_grads: bool = True):
    """Backward of ``switch_ln`` from x alone (smoe_switch_ln_bwd): (dx f32 like x, dweights f32 [K, d], dbiases f32 [K, d]); the
    per-bucket sums are deterministic and an empty bucket's rows are exact zeros.  ``want_param_grads`` False: (dx, None, None)."""
    _chk(x, "x", torch.float32)
    _chk(dy, "dy", align=8)
    dtype_code(dy.dtype)
    d = x.shape[-1]
    T = x.numel() // d if d else 0
    if dy.shape != x.shape or dy.device != x.device:
        raise RuntimeError("switch_ln_bwd: dy must have x's shape")
    K = _switch_ln_tables(x, weights, None, None)
    if K is None:
        K = num_buckets
    if K is None or not switch_ln_supported(d, K):
        raise RuntimeError(f"switch_ln_bwd: d={d}, K={K} outside the kernel's reach")
    _chk(buckets, "buckets", torch.int64, align=8)
    if buckets.numel() != T or buckets.device != x.device:
        raise RuntimeError("switch_ln_bwd: buckets must be int64 of x.shape[:-1] on x's device")
    lib = _lib.load()
    dx = torch.empty_like(x)
    dwb = torch.empty((2, K, d), dtype=torch.float32, device=x.device) if want_param_grads else None
    ws_bytes = lib.smoe_switch_ln_bwd_workspace_bytes(T, d, K)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    with _timed("switch_ln_bwd", {"bytes": T * d * (12 + 2 * dy.element_size())}, x):
        rc = lib.smoe_switch_ln_bwd(_ptr(x), _ptr(dy), dtype_code(dy.dtype), _ptr(weights), _ptr(buckets), float(eps), T, d, K, _ptr(dx),
                                    _ptr(dwb[0]) if want_param_grads else None, _ptr(dwb[1]) if want_param_grads else None,
                                    _ptr(ws), ws_bytes, _stream(x))
    _lib.check(rc, "smoe_switch_ln_bwd")
    if not want_param_grads:
        return dx, None, None
    return dx, dwb[0], dwb[1]
