"""The reference side of tests/test_gpu_nonfinite.py, checked against itself on the CPU.

Every case of the GPU module is a row of CASES: a kernel family, its parameters, ONE input tensor and the position in it that
receives a poison (+inf, -inf, NaN).  A family brings three functions -- the seeded ordinary inputs, the float64 reference of
the operation on (possibly poisoned) inputs, and the hand-written DEPENDENCY CONE: the output elements that depend on the
poisoned position.  The GPU module asserts that nothing outside the cone moves by a bit and that everything the reference
makes non-finite is non-finite on the device, so a wrong cone would make it vacuous (too large: leaks hide) or red for no
reason (too small).  Here the cone is therefore compared with the reference's own behaviour: the set of positions where the
float64 results differ between the poisoned input and two finite substitutes must EQUAL the cone, every containment case must
leave something outside its cone and every propagation case must make the reference non-finite somewhere.

Nothing here needs a GPU or the library; the GPU module imports this module for its cases and references."""
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
FMAX = {torch.float16: 65504.0, torch.bfloat16: 3.3895313892515355e38, torch.float32: 3.4028234663852886e38}
POISONS = ("+inf", "-inf", "nan")
SUBS = (0.75, -1.5)           # the two finite stand-ins of the containment runs
NAN_F32_ALL_ONES = 0x7FFFFFFF  # the f32 NaN whose integer round-to-bf16 carries into the sign bit (a NaN that stores as -0)


def f32_bits(bits: int) -> torch.Tensor:
    return torch.tensor([bits - (1 << 32) if bits >= (1 << 31) else bits], dtype=torch.int32).view(torch.float32)[0]


def poison_value(name, dtype) -> torch.Tensor:
    """0-dim tensor of ``dtype``.  The NaN of an f32 input is the all-ones payload: a conversion that rounds a NaN's bits as if
    they were a number turns exactly this one into a zero."""
    if name == "nan":
        return f32_bits(NAN_F32_ALL_ONES) if dtype == torch.float32 else torch.tensor(float("nan"), dtype=dtype)
    if name in ("+inf", "-inf"):
        return torch.tensor(float("inf") if name == "+inf" else float("-inf"), dtype=dtype)
    return torch.tensor(float(name), dtype=dtype)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def put(inp, target, where, value):
    """A copy of the inputs with ``inp[target][where] = value`` (bit-preserving for a 0-dim tensor of the same dtype)."""
    out = dict(inp)
    t = inp[target].clone()
    t[where] = value.to(t.dtype) if isinstance(value, torch.Tensor) else value
    out[target] = t
    return out


def gelu64(x):
    return torch.nn.functional.gelu(x.double())


def gelu_grad64(h):
    """d/dh gelu(h) = Phi(h) + h phi(h) in float64, as torch's backward forms it (NaN at +-inf: inf * 0)."""
    h = h.double()
    return 0.5 * (1.0 + torch.erf(h * math.sqrt(0.5))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


def cast_like(ref64, dtype):
    """The float64 reference as the kernel's output dtype would hold it."""
    return ref64.to(dtype)


Case = namedtuple("Case", "fam p target where tag propagates")


def case(fam, p, target, where, tag, propagates=True):
    return Case(fam, p, target, where if isinstance(where, tuple) else (where,), tag, propagates)


# ============================================================================================ grouped GEMM
GEMM_COUNTS = (330, 1, 0, 70)      # 255 / 256 and 319 / 320 inside group 0, a one-row group next to an empty one
GEMM_PAD = 7                       # rows past offsets[E]: allocated, never touched


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


class Gemm:
    """out[orow(r)] = [residual[orow] +] [row_scale[orow] *] epi(A[src(r)] W[e]^T + bias[e]); epi GELU_GRAD multiplies by gelu'(H[r])."""

    @staticmethod
    def inputs(p):
        counts, K, N = p.get("counts", GEMM_COUNTS), p.get("K", 128), p.get("N", 72)
        cd, od = DT[p["cd"]], DT[p["od"]]
        offs = _offsets(counts)
        M, E = int(offs[-1]), len(counts)
        g = gen(1000 + M + K + N)
        mode = p.get("mode", "plain")
        inp = {"offsets": torch.from_numpy(offs.astype(np.int32))}
        if mode == "a_gather":
            T = (M + 1) // 2 + 3
            inp["A"] = torch.randn(T, K, generator=g).to(cd)
            inp["a_gather"] = torch.randperm(2 * T, generator=g)[:M].contiguous()
        else:
            inp["A"] = torch.randn(M + GEMM_PAD, K, generator=g).to(cd)
        inp["W"] = (torch.randn(E, N, K, generator=g) * 0.05).to(cd)
        inp["bias"] = torch.randn(E, N, generator=g) * 0.1
        rows = M + GEMM_PAD
        if mode in ("row_map", "row_map_scale", "row_map_scale_residual", "row_map_scale_residual_inplace"):
            inp["row_map"] = torch.randperm(M, generator=g).contiguous()
        if "scale" in mode:
            inp["row_scale"] = torch.rand(rows, generator=g) * 0.75 + 0.25
        if "residual" in mode:
            inp["residual"] = torch.randn(rows, N, generator=g).to(od)
        if p.get("epi") == "gelu_grad":
            inp["H"] = (torch.randn(rows, N, generator=g) * 1.5).to(od)
        if p.get("group_end"):      # separate row ranges: every group ends 3 rows before the next one starts
            inp["group_end"] = torch.from_numpy(np.maximum(offs[1:] - 3, offs[:-1]).astype(np.int32))
        return inp

    @staticmethod
    def _groups(inp):
        offs = inp["offsets"].tolist()
        if "group_end" in inp:
            return [(offs[g], int(inp["group_end"][g])) for g in range(inp["group_end"].numel())]
        return [(offs[g], offs[g + 1]) for g in range(len(offs) - 1)]

    @staticmethod
    def out_init(inp, p):
        """what `out` holds before the launch: the residual when the store is in place, a sentinel otherwise"""
        od = DT[p["od"]]
        if p.get("mode", "").endswith("inplace"):
            return inp["residual"].clone()
        rows = inp["offsets"][-1].item() + GEMM_PAD if "a_gather" not in inp else inp["a_gather"].numel() + GEMM_PAD
        return torch.full((rows, inp["W"].shape[1]), 7.0, dtype=od)

    @staticmethod
    def ref(inp, p):
        out = Gemm.out_init(inp, p).double()
        A, W, bias = inp["A"].double(), inp["W"].double(), inp["bias"].double() if p.get("bias", True) else None
        for e, (lo, hi) in enumerate(Gemm._groups(inp)):
            if hi <= lo:
                continue
            r = torch.arange(lo, hi)
            src = inp["a_gather"][r] // 2 if "a_gather" in inp else r
            v = A[src] @ W[e].t()
            if bias is not None:
                v = v + bias[e]
            if p.get("epi") == "gelu":
                v = gelu64(v)
            elif p.get("epi") == "gelu_grad":
                v = v * gelu_grad64(inp["H"][r])
            orow = inp["row_map"][r] if "row_map" in inp else r
            if "row_scale" in inp:
                v = v * inp["row_scale"][orow].double()[:, None]
            if "residual" in inp:
                v = inp["residual"][orow].double() + v
            out[orow] = v
        return {"out": out}

    @staticmethod
    def out_dtypes(p):
        return {"out": DT[p["od"]]}

    @staticmethod
    def cone(inp, p, target, where):
        out = torch.zeros(Gemm.out_init(inp, p).shape, dtype=torch.bool)
        groups = Gemm._groups(inp)
        live = torch.zeros(out.shape[0], dtype=torch.bool)     # GEMM rows that belong to a group
        for lo, hi in groups:
            live[lo:hi] = True
        orow = lambda r: int(inp["row_map"][r]) if "row_map" in inp else r
        if target == "A":
            t = where[0]
            rows = ([r for r in range(inp["a_gather"].numel()) if int(inp["a_gather"][r]) // 2 == t] if "a_gather" in inp else [t])
            for r in rows:
                if r < live.numel() and live[r]:
                    out[orow(r)] = True
        elif target in ("W", "bias"):
            lo, hi = groups[where[0]]
            for r in range(lo, hi):
                out[orow(r), where[1]] = True
        elif target == "row_scale":
            inv = {orow(r): r for r in range(live.numel()) if live[r]}
            if where[0] in inv:
                out[where[0]] = True
        elif target == "residual":
            inv = {orow(r): r for r in range(live.numel()) if live[r]}
            if where[0] in inv or p["mode"].endswith("inplace"):
                out[where[0], where[1]] = True
        elif target == "H":
            if live[where[0]]:
                out[where[0], where[1]] = True
        else:
            raise KeyError(target)
        return {"out": out}


class GeluKeep:
    """(pre, out) = (A W^T + b, gelu(A W^T + b)), both in the operand dtype"""

    @staticmethod
    def inputs(p):
        return Gemm.inputs(dict(p, od=p["cd"]))

    @staticmethod
    def ref(inp, p):
        q = dict(p, od=p["cd"])
        return {"pre": Gemm.ref(inp, q)["out"], "out": Gemm.ref(inp, dict(q, epi="gelu"))["out"]}

    @staticmethod
    def out_dtypes(p):
        return {"pre": DT[p["cd"]], "out": DT[p["cd"]]}

    @staticmethod
    def cone(inp, p, target, where):
        c = Gemm.cone(inp, dict(p, od=p["cd"]), target, where)["out"]
        return {"pre": c, "out": c.clone()}


# ============================================================================================ weight gradients, column sums
WGRAD_COUNTS = (70, 1, 0, 129, 37)


class Wgrad:
    """out[e] = P[rows of e]^T Q[rows of e], f32 [E, R1, R2] (token-major kernel with S row pieces, or the K-major one)"""

    @staticmethod
    def inputs(p):
        offs = _offsets(p.get("counts", WGRAD_COUNTS))
        n, R1, R2 = int(offs[-1]), p.get("R1", 136), p.get("R2", 72)
        g = gen(4242 + n)
        cd = DT[p["cd"]]
        return {"offsets": torch.from_numpy(offs.astype(np.int32)),
                "P": (torch.randn(n + GEMM_PAD, R1, generator=g) * 0.5).to(cd), "Q": (torch.randn(n + GEMM_PAD, R2, generator=g) * 0.5).to(cd)}

    @staticmethod
    def ref(inp, p):
        o = inp["offsets"].tolist()
        P, Q = inp["P"].double(), inp["Q"].double()
        return {"out": torch.stack([P[o[e]:o[e + 1]].t() @ Q[o[e]:o[e + 1]] for e in range(len(o) - 1)])}

    @staticmethod
    def out_dtypes(p):
        return {"out": torch.float32}

    @staticmethod
    def cone(inp, p, target, where):
        o = inp["offsets"].tolist()
        c = torch.zeros(len(o) - 1, inp["P"].shape[1], inp["Q"].shape[1], dtype=torch.bool)
        r, col = where
        for e in range(len(o) - 1):
            if o[e] <= r < o[e + 1]:
                if target == "P":
                    c[e, col, :] = True
                else:
                    c[e, :, col] = True
        return {"out": c}


class Colsum:
    """out[e, c] = sum over the rows of group e of src[:, c], f32"""

    @staticmethod
    def inputs(p):
        offs = _offsets(p.get("counts", WGRAD_COUNTS))
        n = int(offs[-1])
        return {"offsets": torch.from_numpy(offs.astype(np.int32)),
                "src": (torch.randn(n + GEMM_PAD, p.get("C", 72), generator=gen(77 + n)) * 0.5).to(DT[p["cd"]])}

    @staticmethod
    def ref(inp, p):
        o = inp["offsets"].tolist()
        s = inp["src"].double()
        return {"out": torch.stack([s[o[e]:o[e + 1]].sum(0) for e in range(len(o) - 1)])}

    @staticmethod
    def out_dtypes(p):
        return {"out": torch.float32}

    @staticmethod
    def cone(inp, p, target, where):
        o = inp["offsets"].tolist()
        c = torch.zeros(len(o) - 1, inp["src"].shape[1], dtype=torch.bool)
        for e in range(len(o) - 1):
            if o[e] <= where[0] < o[e + 1]:
                c[e, where[1]] = True
        return {"out": c}


# ============================================================================================ attention
class AttnFwd:
    """out [B, N, H*64] = softmax(q k^T scale) v from qkv [B, N, 3, H, 64]; lse [B, H, N] = log2 of the softmax normaliser"""
    scale = 64 ** -0.5

    @staticmethod
    def inputs(p):
        B, N, H = p["B"], p["N"], p["H"]
        g = gen(B * 1000 + N + H)
        qkv = torch.randn(B, N, 3, H, 64, generator=g) * 1.2
        return {"qkv": qkv.to(DT[p["dt"]])}

    @staticmethod
    def _fwd(qkv64, p):
        B, N, H = p["B"], p["N"], p["H"]
        q, k, v = qkv64.permute(2, 0, 3, 1, 4).unbind(0)
        s = q @ k.transpose(-2, -1) * AttnFwd.scale
        out = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, N, H * 64)
        return out, torch.logsumexp(s, -1) / math.log(2.0)

    @staticmethod
    def ref(inp, p):
        out, lse = AttnFwd._fwd(inp["qkv"].double(), p)
        return {"out": out, "lse": lse} if p.get("lse") else {"out": out}

    @staticmethod
    def out_dtypes(p):
        return {"out": DT[p["dt"]], "lse": torch.float32} if p.get("lse") else {"out": DT[p["dt"]]}

    @staticmethod
    def cone(inp, p, target, where):
        B, N, H = p["B"], p["N"], p["H"]
        b, n, which, h = where[0], where[1], where[2], where[3]
        out = torch.zeros(B, N, H * 64, dtype=torch.bool)
        lse = torch.zeros(B, H, N, dtype=torch.bool)
        rows = [n] if isinstance(n, int) else list(range(N))[n]
        cols = slice(h * 64, h * 64 + 64)
        if which == 0:               # a query row: its own output row
            for r in rows:
                out[b, r, cols] = True
                lse[b, h, r] = True
        elif which == 1:             # a key: every query of the (image, head)
            out[b, :, cols] = True
            lse[b, h, :] = True
        else:                        # a value element: the poisoned head-dim columns of every query; the normaliser never sees v
            c = where[4] if len(where) > 4 else slice(None)
            out[b, :, cols][:, c] = True
        return {"out": out, "lse": lse} if p.get("lse") else {"out": out}


class AttnBwd:
    """dqkv of the above for an upstream dout [B, N, H*64] (float64 autograd of the explicit softmax form)"""

    @staticmethod
    def inputs(p):
        inp = AttnFwd.inputs(p)
        inp["dout"] = (torch.randn(p["B"], p["N"], p["H"] * 64, generator=gen(9 + p["N"])) * 0.5).to(DT[p["dt"]])
        return inp

    @staticmethod
    def ref(inp, p):
        qr = inp["qkv"].double().requires_grad_(True)
        out, _ = AttnFwd._fwd(qr, p)
        out.backward(inp["dout"].double())
        return {"dqkv": qr.grad}

    @staticmethod
    def out_dtypes(p):
        return {"dqkv": DT[p["dt"]]}

    @staticmethod
    def cone(inp, p, target, where):
        B, N, H = p["B"], p["N"], p["H"]
        c = torch.zeros(B, N, 3, H, 64, dtype=torch.bool)
        if target == "dout":
            b, n, col = where
            h = col // 64
            c[b, n, 0, h] = True       # dq of that query
            c[b, :, 1, h] = True       # dk: dS[n, :] moves
            c[b, :, 2, h, col % 64] = True   # dv[:, col] = P^T dO[:, col]
            return {"dqkv": c}
        b, n, which, h = where[0], where[1], where[2], where[3]
        if which == 0:                 # a query row: its dq, and every dk / dv of the head
            c[b, n, 0, h] = True
            c[b, :, 1:, h] = True
        elif which == 1:               # a key row: every probability of the (image, head) moves, so everything of it does
            c[b, :, :, h] = True
        else:                          # a value row: dP = dO V^T moves every dS, hence dq and dk; dv = P^T dO never sees v
            c[b, :, :2, h] = True
        return {"dqkv": c}


# ============================================================================================ LayerNorm
LN_T = 37


class LnFwd:
    """y = (x - mean) rstd g + b over the last dim, f32 in, f32 / 16-bit out (d < 768: 16 lanes per token; d >= 768: a wave per row)"""

    @staticmethod
    def inputs(p):
        d = p["d"]
        g = gen(d)
        return {"x": torch.randn(LN_T, d, generator=g) * 3 + 1, "w": 1 + 0.3 * torch.randn(d, generator=g), "b": 0.2 * torch.randn(d, generator=g)}

    @staticmethod
    def ref(inp, p):
        return {"y": torch.nn.functional.layer_norm(inp["x"].double(), (p["d"],), inp["w"].double(), inp["b"].double(), 1e-6)}

    @staticmethod
    def out_dtypes(p):
        return {"y": DT[p["od"]]}

    @staticmethod
    def cone(inp, p, target, where):
        c = torch.zeros(LN_T, p["d"], dtype=torch.bool)
        if target == "x":
            c[where[0]] = True
        else:                      # an element of the affine weight / bias: its column
            c[:, where[0]] = True
        return {"y": c}


class LnBwd:
    """(dx, dw, db) of the above from x and dy (float64 autograd)"""

    @staticmethod
    def inputs(p):
        inp = LnFwd.inputs(p)
        inp["dy"] = (torch.randn(LN_T, p["d"], generator=gen(p["d"] + 1)) * 0.1).to(DT[p["dyt"]])
        return inp

    @staticmethod
    def ref(inp, p):
        xr, wr, br = (inp[k].double().requires_grad_(True) for k in ("x", "w", "b"))
        torch.nn.functional.layer_norm(xr, (p["d"],), wr, br, 1e-6).backward(inp["dy"].double())
        return {"dx": xr.grad, "dw": wr.grad, "db": br.grad}

    @staticmethod
    def out_dtypes(p):
        return {"dx": torch.float32, "dw": torch.float32, "db": torch.float32}

    @staticmethod
    def cone(inp, p, target, where):
        d = p["d"]
        dx, dw, db = torch.zeros(LN_T, d, dtype=torch.bool), torch.zeros(d, dtype=torch.bool), torch.zeros(d, dtype=torch.bool)
        dx[where[0]] = True            # the row, for a poison in x or in dy
        if target == "dy":             # dw[c] = sum_t dy[t, c] xhat[t, c], db[c] = sum_t dy[t, c]: the poisoned column
            dw[where[1]] = True
            db[where[1]] = True
        else:                          # x: the whole row of xhat moves, so every column of dw; db never sees x
            dw[:] = True
        return {"dx": dx, "dw": dw, "db": db}


# ============================================================================================ rowdot (the combine scores' gradient)
class Rowdot:
    """dscore[i] = <dout[i // k], y[inv_pos[i]]>, 0 for a dropped entry (inv_pos[i] < 0); f32"""
    T, K_TOP, D = 41, 2, 192

    @staticmethod
    def inputs(p):
        g = gen(313)
        T, k, d = Rowdot.T, Rowdot.K_TOP, Rowdot.D
        inv = torch.randperm(T * k + 9, generator=g)[:T * k].contiguous()
        inv[2 * 5] = -1              # token 5 lost one of its two entries to the capacity gate ...
        inv[2 * 7] = inv[2 * 7 + 1] = -1     # ... token 7 both
        dt = DT[p["dt"]]
        return {"dout": torch.randn(T, d, generator=g).to(dt), "y": torch.randn(T * k + 9, d, generator=g).to(dt), "inv_pos": inv}

    @staticmethod
    def ref(inp, p):
        inv = inp["inv_pos"]
        tok = torch.arange(inv.numel()) // Rowdot.K_TOP
        val = (inp["dout"].double()[tok] * inp["y"].double()[inv.clamp(min=0)]).sum(-1)
        return {"dscore": torch.where(inv >= 0, val, torch.zeros_like(val))}

    @staticmethod
    def out_dtypes(p):
        return {"dscore": torch.float32}

    @staticmethod
    def cone(inp, p, target, where):
        inv = inp["inv_pos"]
        i = torch.arange(inv.numel())
        if target == "dout":
            return {"dscore": (i // Rowdot.K_TOP == where[0]) & (inv >= 0)}
        return {"dscore": inv == where[0]}


def _rowdot_cases():
    out = []
    for dt in ("f16", "bf16"):
        p = dict(dt=dt)
        out.append(case("rowdot", p, "dout", (0, 0), f"{dt}-dout[0,0]"))
        out.append(case("rowdot", p, "dout", (Rowdot.T - 1, Rowdot.D - 1), f"{dt}-dout[last,last]"))
        out.append(case("rowdot", p, "dout", (5, 8), f"{dt}-dout[token with one dropped entry]"))
        out.append(case("rowdot", p, "dout", (7, 8), f"{dt}-dout[token the capacity gate drops]", propagates=False))
        inp = Rowdot.inputs(p)
        live = int(inp["inv_pos"][0])
        unused = sorted(set(range(inp["y"].shape[0])) - set(inp["inv_pos"].tolist()))[0]
        out.append(case("rowdot", p, "y", (live, Rowdot.D - 8), f"{dt}-y[a routed row,last vector]"))
        out.append(case("rowdot", p, "y", (unused, 3), f"{dt}-y[a row no entry points to]", propagates=False))
    return out


FAMILIES = {"rowdot": Rowdot, "gemm": Gemm, "gelu_keep": GeluKeep, "wgrad": Wgrad, "colsum": Colsum, "attn_fwd": AttnFwd, "attn_bwd": AttnBwd,
            "ln_fwd": LnFwd, "ln_bwd": LnBwd}


# ============================================================================================ the table
def _gemm_cases():
    out = []
    K, N = 128, 72
    M = sum(GEMM_COUNTS)
    edge_rows = (0, 255, 256, 319, 320, 329, 330, 331, M - 1)
    # every edge row, last column of A, per kernel structure (f16 in, f16 out): 0 register-staged, 4 one workgroup per tile,
    # 9 persistent + direct store, 10 / 13 forced 320-row tile (13: deep schedule), 14 persistent + staged epilogue
    for variant in (0, 4, 9, 10, 13, 14):
        p = dict(variant=variant, cd="f16", od="f16", epi="none")
        for r in edge_rows:
            out.append(case("gemm", p, "A", (r, K - 1), f"v{variant}-f16-f16-none-A[{r},last]"))
        out.append(case("gemm", p, "A", (M + 2, 0), f"v{variant}-f16-f16-none-A[past offsets[E]]", propagates=False))
    # operand / output dtypes and epilogues at the rows either side of the two tile heights and in the one-row group
    for variant in (0, 4, 9, 10, 14):
        for cd in ("f16", "bf16"):
            for od in ("f16", "bf16", "f32"):
                if od in ("f16", "bf16") and od != cd:
                    continue
                for epi in ("none", "gelu", "gelu_grad"):
                    p = dict(variant=variant, cd=cd, od=od, epi=epi)
                    t = f"v{variant}-{cd}-{od}-{epi}"
                    out.append(case("gemm", p, "A", (255, 0), f"{t}-A[255,0]"))
                    out.append(case("gemm", p, "A", (320, K - 8), f"{t}-A[320,last vector]"))
                    out.append(case("gemm", p, "W", (1, N - 1, 5), f"{t}-W[one-row expert,last column]"))
                    out.append(case("gemm", p, "bias", (0, N - 8), f"{t}-bias[0,last vector]"))
                    if epi == "gelu_grad":
                        out.append(case("gemm", p, "H", (319, N - 1), f"{t}-H[319,last]"))
                        out.append(case("gemm", p, "H", (330, 0), f"{t}-H[one-row group]"))
    # the fused combine / residual / scatter forms
    for variant in (0, 4, 9, 10, 14):
        for cd, od in (("f16", "f32"), ("bf16", "f32"), ("f16", "f16"), ("bf16", "bf16")):
            for mode in ("row_map", "row_map_scale", "row_map_scale_residual", "row_map_scale_residual_inplace", "residual", "a_gather"):
                if mode == "a_gather" and variant == 0:
                    continue
                p = dict(variant=variant, cd=cd, od=od, epi="none", mode=mode)
                t = f"v{variant}-{cd}-{od}-{mode}"
                if mode == "a_gather":
                    out.append(case("gemm", p, "A", (3, 1), f"{t}-A[token 3]"))
                    out.append(case("gemm", p, "A", (M // 2 + 1, K - 1), f"{t}-A[late token]"))
                    continue
                out.append(case("gemm", p, "A", (256, 1), f"{t}-A[256]"))
                out.append(case("gemm", p, "A", (330, 1), f"{t}-A[one-row group]"))
                if "scale" in mode:
                    out.append(case("gemm", p, "row_scale", (17,), f"{t}-row_scale[17]"))
                if "residual" in mode:
                    out.append(case("gemm", p, "residual", (M - 1, N - 1), f"{t}-residual[last,last]"))
    # separate row ranges (persistent kernel only): live rows at both ends of a range, and the gap rows nobody owns
    for variant in (9, 10, 14):
        for od in ("f16", "f32"):
            p = dict(variant=variant, cd="f16", od=od, epi="gelu", group_end=True)
            t = f"v{variant}-f16-{od}-ranges"
            out.append(case("gemm", p, "A", (326, 0), f"{t}-A[last live row of range 0]"))
            out.append(case("gemm", p, "A", (327, 0), f"{t}-A[gap after range 0]", propagates=False))
            out.append(case("gemm", p, "A", (330, 0), f"{t}-A[the one-row group, emptied]", propagates=False))
            out.append(case("gemm", p, "A", (331, 0), f"{t}-A[first row of the last range]"))
    for cd in ("f16", "bf16"):
        p = dict(cd=cd, od=cd)
        for r in (0, 255, 256, 319, 320, 330, M - 1):
            out.append(case("gelu_keep", p, "A", (r, K - 1), f"{cd}-A[{r},last]"))
        out.append(case("gelu_keep", p, "W", (3, N - 1, 0), f"{cd}-W[3,last column]"))
        out.append(case("gelu_keep", p, "bias", (1, 0), f"{cd}-bias[one-row expert]"))
        out.append(case("gelu_keep", p, "A", (M + 1, 0), f"{cd}-A[past offsets[E]]", propagates=False))
    return out


def _wgrad_cases():
    out = []
    n = sum(WGRAD_COUNTS)
    for cd in ("f16", "bf16"):
        for S in (1, 4):
            p = dict(cd=cd, S=S)
            for r in (0, 63, 64, 69, 70, 71, 71 + 63, 71 + 64, n - 1):
                out.append(case("wgrad", p, "P", (r, 135), f"{cd}-S{S}-P[{r},last]"))
            out.append(case("wgrad", p, "Q", (70, 71), f"{cd}-S{S}-Q[one-row expert,last]"))
            out.append(case("wgrad", p, "Q", (n + 1, 0), f"{cd}-S{S}-Q[past offsets[E]]", propagates=False))
        for S in range(2, 17):     # every piece count ops.expert_wgrad_splits can pick
            if S != 4:
                out.append(case("wgrad", dict(cd=cd, S=S), "P", (71 + 64, 8), f"{cd}-S{S}-P[piece boundary]"))
        p = dict(cd=cd, kmajor=True)
        for r in (0, 69, 70, 71, n - 1):
            out.append(case("wgrad", p, "P", (r, 135), f"{cd}-kmajor-P[{r},last]"))
        out.append(case("wgrad", p, "Q", (199, 7), f"{cd}-kmajor-Q[199,7]"))
        for r in (0, 69, 70, 71, n - 1):
            out.append(case("colsum", dict(cd=cd), "src", (r, 71), f"{cd}-src[{r},last]"))
        out.append(case("colsum", dict(cd=cd), "src", (n + 3, 0), f"{cd}-src[past offsets[E]]", propagates=False))
    return out


def _attn_cases():
    out = []
    for dt in ("f16", "bf16"):
        # short kernel: N = 197 (the exact 13-tile form), 50 (general mask form), 256 (no partial tile), with and without lse
        for N, lse in ((197, True), (197, False), (50, True), (256, False)):
            p = dict(B=2, N=N, H=3, dt=dt, lse=lse)
            t = f"{dt}-N{N}{'-lse' if lse else ''}"
            out.append(case("attn_fwd", p, "qkv", (1, N - 1, 0, 2, 63), f"{t}-q[last row]"))
            out.append(case("attn_fwd", p, "qkv", (0, 0, 1, 1, 0), f"{t}-k[key 0]"))
            out.append(case("attn_fwd", p, "qkv", (1, N - 1, 1, 0, 7), f"{t}-k[key N-1, the duplicated row]"))
            out.append(case("attn_fwd", p, "qkv", (0, N - 3, 1, 2, 63), f"{t}-k[last partial tile]"))
            out.append(case("attn_fwd", p, "qkv", (1, N - 1, 2, 1, 5), f"{t}-v[key N-1]"))
            out.append(case("attn_fwd", p, "qkv", (0, 0, 2, 0, 63), f"{t}-v[key 0]"))
        # long kernel (online softmax)
        for N in (257, 577, 640):
            p = dict(B=1, N=N, H=2, dt=dt)
            t = f"{dt}-N{N}"
            out.append(case("attn_fwd", p, "qkv", (0, N - 1, 0, 1, 0), f"{t}-q[last row]"))
            out.append(case("attn_fwd", p, "qkv", (0, 0, 1, 0, 3), f"{t}-k[key 0]"))
            out.append(case("attn_fwd", p, "qkv", (0, N - 1, 1, 1, 63), f"{t}-k[key N-1]"))
            out.append(case("attn_fwd", p, "qkv", (0, N - 2, 2, 0, 9), f"{t}-v[last partial tile]"))
            # column 11 of the first chunk's 160 keys: -inf there makes EVERY score of the chunk -inf for queries with q[11] > 0
            out.append(case("attn_fwd", p, "qkv", (0, slice(0, 160), 1, 1, 11), f"{t}-k[first chunk,col 11]"))
        for N, waves in ((197, 8), (197, 4), (50, 4), (100, 8), (100, 4), (256, 8)):
            p = dict(B=2, N=N, H=2, dt=dt, waves=waves)
            t = f"{dt}-N{N}-w{waves}"
            out.append(case("attn_bwd", p, "qkv", (1, N - 1, 0, 1, 63), f"{t}-q[last row]"))
            out.append(case("attn_bwd", p, "qkv", (0, 0, 1, 0, 0), f"{t}-k[key 0]"))
            out.append(case("attn_bwd", p, "qkv", (1, N - 1, 1, 0, 7), f"{t}-k[key N-1]"))
            out.append(case("attn_bwd", p, "qkv", (0, N - 1, 2, 1, 5), f"{t}-v[key N-1]"))
            out.append(case("attn_bwd", p, "dout", (1, N - 1, 64 + 3), f"{t}-dout[last row]"))
            out.append(case("attn_bwd", p, "dout", (0, 0, 0), f"{t}-dout[0,0]"))
    return out


def _ln_cases():
    out = []
    for d in (192, 384, 768, 1024):          # both layouts (SMOE_LN_WAVE's default: 16 lanes per token below 768, a wave per row from there)
        for od in ("f32", "f16", "bf16"):
            p = dict(d=d, od=od)
            for t, col in ((0, 0), (LN_T - 1, d - 1), (15, d - 8), (16, 5)):     # first / last row, the rows either side of a 16-token group
                out.append(case("ln_fwd", p, "x", (t, col), f"d{d}-{od}-x[{t},{col}]"))
            out.append(case("ln_fwd", p, "w", (d - 1,), f"d{d}-{od}-w[last]"))
            out.append(case("ln_fwd", p, "b", (0,), f"d{d}-{od}-b[0]"))
        for dyt in ("f32", "f16"):
            p = dict(d=d, dyt=dyt)
            for t, col in ((0, 0), (LN_T - 1, d - 1), (16, d - 8)):
                out.append(case("ln_bwd", p, "x", (t, col), f"d{d}-dy {dyt}-x[{t},{col}]"))
                out.append(case("ln_bwd", p, "dy", (t, col), f"d{d}-dy {dyt}-dy[{t},{col}]"))
    return out


CASES = _gemm_cases() + _wgrad_cases() + _attn_cases() + _ln_cases() + _rowdot_cases()


def case_id(c):
    return f"{c.fam}:{c.tag}"


def cases_of(*fams):
    return [c for c in CASES if c.fam in fams]


_inputs_cache = {}


def inputs_of(c):
    key = (c.fam, tuple(sorted((k, str(v)) for k, v in c.p.items())))
    if key not in _inputs_cache:
        if len(_inputs_cache) > 8:
            _inputs_cache.clear()
        _inputs_cache[key] = FAMILIES[c.fam].inputs(c.p)
    return _inputs_cache[key]


def differs(a, b):
    """positions where two float64 results are not the same value (two NaNs count as the same)"""
    return ~((a == b) | (torch.isnan(a) & torch.isnan(b)))


# ============================================================================================ the checks
def test_the_table_is_not_empty_and_ids_are_unique():
    ids = [case_id(c) for c in CASES]
    assert len(ids) == len(set(ids)) and len(ids) > 500, len(ids)
    for fam in FAMILIES:
        assert cases_of(fam), fam


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_hand_written_cone_equals_the_reference_dependency_set(fam):
    """For every case: {positions where the f64 reference differs between the poisoned and the substituted inputs} == cone, for each
    of the three poisons; a containment case leaves at least one element outside its cone; a propagation case has at least one
    non-finite reference element after the cast to the kernel's output dtype."""
    F = FAMILIES[fam]
    for c in cases_of(fam):
        inp = inputs_of(c)
        cone = F.cone(inp, c.p, c.target, c.where)
        dts = F.out_dtypes(c.p)
        dt_in = inp[c.target].dtype
        subs = [F.ref(put(inp, c.target, c.where, s), c.p) for s in SUBS]
        assert set(cone) == set(subs[0]) == set(dts), case_id(c)
        assert any((~m).any() for m in cone.values()), f"{case_id(c)}: nothing outside the cone, containment is vacuous"
        for name in POISONS:
            bad = F.ref(put(inp, c.target, c.where, poison_value(name, dt_in)), c.p)
            nonfinite = 0
            for k, m in cone.items():
                moved = differs(bad[k], subs[0][k]) | differs(bad[k], subs[1][k]) | differs(subs[0][k], subs[1][k])
                assert moved.shape == m.shape, (case_id(c), k)
                assert torch.equal(moved, m), (f"{case_id(c)} {name} {k}: cone has {int(m.sum())} elements, the reference moves "
                                               f"{int(moved.sum())}; only in cone {int((m & ~moved).sum())}, only moved {int((moved & ~m).sum())}")
                nonfinite += int((~torch.isfinite(cast_like(bad[k], dts[k]))).sum())
                assert torch.isfinite(subs[0][k]).all() and torch.isfinite(subs[1][k]).all(), (case_id(c), k)
            if c.propagates:
                assert nonfinite > 0, f"{case_id(c)} {name}: the reference stays finite, propagation is vacuous"
            else:
                assert not any(m.any() for m in cone.values()) and nonfinite == 0, case_id(c)


def test_first_chunk_case_really_masks_a_whole_chunk_for_some_queries():
    """The long-kernel case must contain queries whose first 160 scores are all -inf while the float64 softmax stays finite."""
    for c in cases_of("attn_fwd"):
        if "first chunk" not in c.tag:
            continue
        inp = put(inputs_of(c), c.target, c.where, poison_value("-inf", inputs_of(c)[c.target].dtype))
        ref = AttnFwd.ref(inp, c.p)["out"]
        h = c.where[3]
        q_col = inp["qkv"][0, :, 0, h, 11].double()
        fin = torch.isfinite(ref[0, :, h * 64:(h + 1) * 64]).all(-1)
        assert torch.equal(fin, q_col > 0) and int(fin.sum()) > 10 and int((~fin).sum()) > 10


# ---- the pieces of the GPU module's non-table tests that have a CPU side ---------------------------------------------------------
def store_expectation(ref64, dtype):
    """(must_be_inf, sign, must_be_nan, must_be_finite) of a 16-bit store of exact values ``ref64``: beyond twice the largest finite
    value the result is inf of the value's sign whatever the rounding mode, below half of it it is finite; NaN stays NaN."""
    big = ref64.abs() >= 2.0 * FMAX[dtype]
    return big & ~torch.isnan(ref64), torch.sign(ref64), torch.isnan(ref64), ref64.abs() <= 0.5 * FMAX[dtype]


def check_store(got, ref64, dtype, what):
    """The 16-bit-store property on a device result (CPU tensors)."""
    must_inf, sign, must_nan, must_fin = store_expectation(ref64, dtype)
    g = got.double()
    sat = must_inf & ~(torch.isinf(g) & (torch.sign(g) == sign))
    assert not sat.any(), (f"{what}: {int(sat.sum())} of {int(must_inf.sum())} overflowing values were not stored as inf of their sign; "
                           f"first: exact {ref64[sat][0].item():.6g} stored as {g[sat][0].item():.6g}")
    lost = must_nan & ~torch.isnan(g)
    assert not lost.any(), f"{what}: {int(lost.sum())} of {int(must_nan.sum())} NaNs were stored as numbers; first stored as {g[lost][0].item():.6g}"
    wrong = must_fin & ~torch.isfinite(g)
    assert not wrong.any(), f"{what}: {int(wrong.sum())} in-range values were stored as non-finite"
    return int(must_inf.sum()), int(must_nan.sum())


NAN_PATTERNS_F32 = (0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001, 0xFF800001, 0x7FBFFFFF, 0xFFBFFFFF, 0x7F80FFFF, 0xFF808000)


def store_vector(dtype):
    """f32 values for the elementwise stores: both sides of the format's range, exact halves, every class of NaN."""
    m = FMAX[dtype]
    big = [2.0 * m, 4.0 * m, 1e38 if dtype == torch.float16 else 3.4e38, float("inf")] if 2.0 * m < FMAX[torch.float32] else [float("inf")]
    fin = [0.0, 1.0, -1.0, 0.25 * m, 0.5 * m]
    vals = torch.tensor([s * v for v in big + fin for s in (1.0, -1.0)], dtype=torch.float32)
    return torch.cat([vals, torch.stack([f32_bits(b) for b in NAN_PATTERNS_F32])])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_store_expectation_agrees_with_torch_round_to_nearest(dtype):
    v = store_vector(dtype)
    assert torch.isnan(v[-len(NAN_PATTERNS_F32):]).all(), "every pattern is a NaN"
    must_inf, sign, must_nan, must_fin = store_expectation(v.double(), dtype)
    assert int(must_nan.sum()) == len(NAN_PATTERNS_F32) and int(must_fin.sum()) >= 8
    assert int(must_inf.sum()) >= (2 if dtype == torch.bfloat16 else 8)
    check_store(v.to(dtype), v.double(), dtype, "torch's own cast")
    with pytest.raises(AssertionError):
        check_store(v.clamp(-FMAX[dtype], FMAX[dtype]).to(dtype), v.double(), dtype, "a saturating cast")
    with pytest.raises(AssertionError):
        check_store(torch.nan_to_num(v, nan=0.0).to(dtype), v.double(), dtype, "a NaN-dropping cast")


def integer_rounded_bf16(v):
    """f32 -> bf16 by integer arithmetic WITHOUT a NaN select (what the library's f32_to_bf16 would be without its select)."""
    u = v.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    return (r << 16).to(torch.int64).apply_(lambda x: x - (1 << 32) if x >= (1 << 31) else x).to(torch.int32).view(torch.float32)


def test_the_nan_patterns_include_the_ones_integer_rounding_loses():
    """Without the select, all-ones payloads carry into the exponent / sign (a NaN becomes +-0) and small signalling payloads round to
    +-inf: the test vector must hold both kinds, or the GPU test could not notice a missing select."""
    pats = torch.stack([f32_bits(b) for b in NAN_PATTERNS_F32])
    r = integer_rounded_bf16(pats)
    assert int((r == 0).sum()) >= 2 and int(torch.isinf(r).sum()) >= 2 and int(torch.isnan(r).sum()) >= 2
    assert float(integer_rounded_bf16(poison_value("nan", torch.float32).reshape(1))[0]) == 0.0


SUMSQ_N = 2 * 16384 + 8 * 5 + 5        # two whole blocks, five whole 8-vectors and a 5-element scalar tail (not a multiple of 4 either)


def sumsq_positions(n=SUMSQ_N):
    tail = n - n % 8
    return [0, 7, 8, 16383, 16384, tail - 1] + list(range(tail, n))


def found_inf_ref(g, inv_scale):
    """GradScaler.unscale_'s flag: any element of g * inv_scale (f32 arithmetic) that is not finite"""
    return float((~torch.isfinite(g.float() * torch.tensor(inv_scale, dtype=torch.float32))).any())


def test_sumsq_positions_cover_the_vector_path_and_every_tail_slot():
    pos = sumsq_positions()
    n = SUMSQ_N
    assert n % 8 == 5 and n % 4 != 0 and 0 in pos and n - 1 in pos
    assert {q for q in pos if q >= n - n % 8} == set(range(n - 5, n)), "each position of the scalar tail"
    assert any(q % 8 == 7 and q < n - n % 8 for q in pos), "the last element of a full 8-vector"
    g = torch.ones(n)
    assert found_inf_ref(g, 1.0) == 0.0
    g[n - 1] = 1e30
    assert found_inf_ref(g, 1.0) == 0.0 and found_inf_ref(g, 1e10) == 1.0, "finite until multiplied by inv_scale"


GELU_SWEEP = (0.0, 1e-3, 0.5, 1.0, 2.5, 4.0, 5.5, 7.9, 8.0, 8.1, 9.0, 12.0, 20.0, 64.0, 300.0, 4096.0, 60000.0, 1e6, 3e38, float("inf"))


def gelu_sweep_values():
    v = torch.tensor(GELU_SWEEP, dtype=torch.float32)
    return torch.cat([v, -v, torch.tensor([float("nan")])])


def test_gelu_references_at_the_ends_of_the_range():
    v = gelu_sweep_values().double()
    y, dy = gelu64(v), gelu_grad64(v)
    assert y[v == float("inf")].item() == float("inf") and torch.isnan(y[v == float("-inf")]).all() and torch.isnan(y[-1])
    assert torch.isnan(dy[torch.isinf(v)]).all() and torch.isnan(dy[-1])
    fin = torch.isfinite(v)
    assert torch.isfinite(y[fin]).all() and torch.isfinite(dy[fin]).all()
    assert (y[fin & (v <= -40)] == 0).all() and (y[fin & (v >= 40)] == v[fin & (v >= 40)]).all()
    hr = v[fin].clone().requires_grad_(True)
    torch.nn.functional.gelu(hr).sum().backward()
    assert (hr.grad - dy[fin]).abs().max().item() <= 1e-12, "gelu_grad64 is torch's float64 derivative"
