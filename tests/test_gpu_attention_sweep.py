"""Every sequence length of the attention kernels (csrc/attention.hip, attention_bwd.hip: N = 1 .. 640; attention_skip.hip: per-image
lengths 1 .. 256 and smoe_skip_plan), forward, backward and varlen, at B = 3, H = 2 in f16 and bf16 (tests/_attn_sweep_cases.py).

Per length: (a) out / lse / dqkv against float64 at the project's existing bars, restated below and pinned to their sources by
test_the_restated_bars_are_the_projects; (b) image 1 and head 0 keep their BITS when the neighbouring images / the other head are
NaN, and image 1 alone in a B = 1 call gives the same bits -- one element read across an image's or head's end and not masked is a
NaN; (c) through the C entry points with caller-owned buffers pre-filled with a NaN payload: the guard bands keep it, no element
inside does; (d) per instantiation (ac.bucket) the largest error / bar ratio and the N it occurred at, printed.

dq and dk at N = 1.  softmax over one key is 1 whatever the score, so dq = dk = 0 analytically (dS = P (dP - delta) with delta =
dP); _assert_bwd's two quotients (|diff| over |ref|) have no denominator there.  At N = 1 ONLY the denominators of dq and dk are
those of the same sum before it cancels, scale |dP| |k| and scale |dP| |q| per element -- the magnitude a kernel that got the single
key's probability or delta wrong would return -- under the same two bars; dv (= dout) and every N >= 2 use the rule as it stands."""
import functools
import hashlib
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import slim_switch_moe_vit_amd as sm  # noqa: E402,F401
from slim_switch_moe_vit_amd import _lib, ops  # noqa: E402

import _attn_sweep_cases as ac  # noqa: E402
import _skip_attn_cases as sc  # noqa: E402

DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
# the project's bars, restated (test_the_restated_bars_are_the_projects holds them to their sources)
OUT_TOL = {F16: 2e-3, BF16: 1.5e-2}          # x max(1, max |ref|): tests/test_gpu_parity.py, the two attention kernel tests
LSE_TOL = {F16: 2e-3, BF16: 2e-2}            # absolute, log2 domain: tests/test_gpu_attention_long.py
BWD_REL = {F16: 9.4e-4, BF16: 7.6e-3}        # relative L2 per dq / dk / dv: tests/test_gpu_attention_long.py::_assert_bwd
BWD_MAX = {F16: 2.4e-3, BF16: 1.7e-2}        # max |diff| / max |ref| per dq / dk / dv: the same
VARLEN_BAR = {F16: 3.0 * 1.078e-3, BF16: 3.0 * 8.467e-3}      # tests/test_gpu_skip_attention.py
GUARD = 4096                                 # elements in front of and behind every caller-owned buffer


def test_the_restated_bars_are_the_projects():
    import inspect
    import test_gpu_attention_long as al
    import test_gpu_parity as par
    import test_gpu_skip_attention as sk
    assert (LSE_TOL, BWD_REL, BWD_MAX, VARLEN_BAR) == (al.LSE_TOL, al.BWD_REL, al.BWD_MAX, sk.VARLEN_BAR)
    assert "(torch.float16, 2e-3), (torch.bfloat16, 1.5e-2)" in inspect.getsource(par)
    assert ac.SCALE == al.SCALE


# ------------------------------------------------------------------------------------------------------------------ helpers
def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _fwd_bwd(qkv, dout):
    Bq, N, _, Hq, _ = qkv.shape
    out, lse = ops.attention(qkv, Bq, N, Hq, 64, ac.SCALE, want_lse=True)
    return out, lse, ops.attention_bwd(qkv, out, dout, lse, Bq, N, Hq, 64, ac.SCALE)


def _dev_inputs(N, dt):
    qkv, dout = ac.inputs(N, dt)
    return qkv.to(DEV), dout.to(DEV)


def _bwd_denominators(ref, qkv, dout):
    """per dq / dk / dv: (||ref||_2, max |ref|) -- at N = 1 for dq / dk those of the uncancelled sum (the module's docstring)"""
    den = [(ref["dqkv"][:, :, i].norm().clamp(min=1e-30), ref["dqkv"][:, :, i].abs().max()) for i in range(3)]
    if qkv.shape[1] == 1:
        Bq, _, _, Hq, hd = qkv.shape
        q, k, v = qkv.double().unbind(2)                                                    # [B, 1, H, hd]
        dp = (dout.double().reshape(Bq, 1, Hq, hd) * v).sum(-1, keepdim=True).abs()          # |dP| [B, 1, H, 1]
        for i, other in ((0, k), (1, q)):
            u = ac.SCALE * dp * other.abs()
            den[i] = (u.norm(), u.max())
    return den


def _ratios(got, ref, qkv, dout, dt):
    """device tensor [8] of error / bar: out, lse, then (relative L2, max / max |ref|) of dq, dk, dv"""
    out, lse, dqkv = got
    r = [(out.double() - ref["out"]).abs().max() / (OUT_TOL[dt] * ref["out"].abs().max().clamp(min=1.0)),
         (lse.double() - ref["lse"]).abs().max() / LSE_TOL[dt]]
    for i, (nrm, mx) in enumerate(_bwd_denominators(ref, qkv, dout)):
        d = dqkv[:, :, i].double() - ref["dqkv"][:, :, i]
        r += [d.norm() / nrm / BWD_REL[dt], d.abs().max() / mx / BWD_MAX[dt]]
    return torch.stack(r)


RATIO_NAMES = ("out", "lse", "dq L2", "dq max", "dk L2", "dk max", "dv L2", "dv max")
CASES = [pytest.param(i, dt, id=f"N{c[0]}-{c[-1]}-{ac.dtype_name(dt)}") for i, c in enumerate(ac.CHUNKS) for dt in ac.DTYPES]


# ---------------------------------------------------------------------------------------------------- (a) values, (d) the report
@pytest.mark.parametrize("chunk,dt", CASES)
def test_every_length_against_float64(chunk, dt):
    ns = list(ac.CHUNKS[chunk])
    rows = []
    for N in ns:
        qkv, dout = _dev_inputs(N, dt)
        rows.append(_ratios(_fwd_bwd(qkv, dout), ac.reference(qkv, dout), qkv, dout, dt))
    ratios = torch.stack(rows).cpu().numpy()                                              # [64, 8] error / bar
    ratios = np.where(np.isnan(ratios), np.inf, ratios)
    by_bucket = {}
    for N, r in zip(ns, ratios):
        by_bucket.setdefault(ac.bucket(N), []).append((N, r))
    for b, items in by_bucket.items():
        worst = []
        for cols, nm in (((0,), "out"), ((1,), "lse"), (tuple(range(2, 8)), "dqkv")):
            w, N = max((max(r[c] for c in cols), N) for N, r in items)
            worst.append(f"{nm} {w:.3f} at N {N}")
        print(f"{ac.dtype_name(dt)} N {items[0][0]}-{items[-1][0]} {b.fwd} / {b.bwd}: worst error / bar  " + "  ".join(worst))
    bad = [(N, RATIO_NAMES[c], float(f"{r[c]:.3f}")) for N, r in zip(ns, ratios) for c in range(8) if not r[c] <= 1.0]
    assert not bad, f"(N, what, error / bar) over the bar: {bad}"


# ------------------------------------------------------------------------------------- (b) neighbour independence, bit for bit
def _poison(t, index):
    _bits(t)[index] = ac.NAN16[t.dtype]


@pytest.mark.parametrize("chunk,dt", CASES)
def test_every_length_keeps_its_bits_beside_nan_images_and_heads(chunk, dt):
    bad = []
    for N in ac.CHUNKS[chunk]:
        qkv, dout = _dev_inputs(N, dt)
        base = _fwd_bwd(qkv, dout)
        if not all(bool(torch.isfinite(t).all()) for t in base):
            bad.append((N, "finite inputs, non-finite result"))
        qp, dp = qkv.clone(), dout.clone()                       # images 0 and 2 are NaN
        for img in (0, 2):
            _poison(qp, img)
            _poison(dp, img)
        got = _fwd_bwd(qp, dp)
        alone = _fwd_bwd(qkv[1:2].contiguous(), dout[1:2].contiguous())
        for nm, b, g, a in zip(("out", "lse", "dqkv"), base, got, alone):
            if not _same(g[1], b[1]):
                bad.append((N, nm, "image 1 changed beside NaN images"))
            if not _same(a[0], b[1]):
                bad.append((N, nm, "image 1 alone (B = 1) differs from image 1 of the batch"))
        qh, dh = qkv.clone(), dout.clone()                       # head 1 of every image is NaN
        _poison(qh, (slice(None), slice(None), slice(None), 1))
        _poison(dh, (slice(None), slice(None), slice(64, 128)))
        out, lse, dqkv = _fwd_bwd(qh, dh)
        for nm, b, g in (("out", base[0][:, :, :64], out[:, :, :64]), ("lse", base[1][:, 0], lse[:, 0]),
                         ("dqkv", base[2][:, :, :, 0], dqkv[:, :, :, 0])):
            if not _same(g, b):
                bad.append((N, nm, "head 0 changed beside a NaN head"))
    assert not bad, f"{bad}"


# ------------------------------------------------------------------------------------- (c) stores stay inside, and cover everything
def _guarded(n, dt):
    """(whole buffer, pointer to its n logical elements) with GUARD payload elements on either side"""
    if dt == torch.float32:
        buf = torch.full((n + 2 * GUARD,), ac.NAN32, dtype=torch.int32, device=DEV)
    else:
        buf = torch.full((n + 2 * GUARD,), ac.NAN16[dt], dtype=torch.int16, device=DEV)
    return buf, buf.data_ptr() + GUARD * buf.element_size()


def _guard_verdict(buf, n, payload):
    """device bools: (both guard bands hold the payload, no element inside does)"""
    bands = (buf[:GUARD] == payload).all() & (buf[GUARD + n:] == payload).all()
    return bands, ~(buf[GUARD:GUARD + n] == payload).any()


@pytest.mark.parametrize("chunk,dt", CASES)
def test_every_length_stores_inside_its_buffers_and_covers_them(chunk, dt):
    lib, code = _lib.load(), ops.dtype_code(dt)
    ns = list(ac.CHUNKS[chunk])
    verdicts, bad = [], []
    for N in ns:
        qkv, dout = _dev_inputs(N, dt)
        n_out, n_lse = ac.B * N * ac.H * 64, ac.B * ac.H * N
        obuf, optr = _guarded(n_out, dt)
        lbuf, lptr = _guarded(n_lse, torch.float32)
        gbuf, gptr = _guarded(3 * n_out, dt)
        assert int(obuf[0]) == ac.NAN16[dt] and optr % 16 == 0 and lptr % 16 == 0 and gptr % 16 == 0
        stream = ops._stream(qkv)
        _lib.check(lib.smoe_attention_fwd(qkv.data_ptr(), optr, code, ac.B, N, ac.H, 64, ac.SCALE, lptr, stream), "smoe_attention_fwd")
        _lib.check(lib.smoe_attention_bwd(qkv.data_ptr(), optr, dout.data_ptr(), lptr, gptr, code, ac.B, N, ac.H, 64, ac.SCALE, stream),
                   "smoe_attention_bwd")
        verdicts.append(torch.stack(_guard_verdict(obuf, n_out, ac.NAN16[dt]) + _guard_verdict(lbuf, n_lse, ac.NAN32)
                                    + _guard_verdict(gbuf, 3 * n_out, ac.NAN16[dt])))
        base = _fwd_bwd(qkv, dout)
        for nm, buf, n, b in (("out", obuf, n_out, base[0]), ("lse", lbuf, n_lse, base[1]), ("dqkv", gbuf, 3 * n_out, base[2])):
            if not torch.equal(buf[GUARD:GUARD + n], _bits(b).reshape(-1)):
                bad.append((N, nm, "the C entry point and ops.* disagree"))
    verdicts = torch.stack(verdicts).cpu().numpy()
    names = ("out guard written", "out element never written", "lse guard written", "lse element never written",
             "dqkv guard written", "dqkv element never written")
    bad += [(N, names[c]) for N, v in zip(ns, verdicts) for c in range(6) if not v[c]]
    assert not bad, f"{bad}"


# ------------------------------------------------------------------------------------------------------------ 4-wave backward
WAVE_NS = range(49, 257)


def _bwd_digests():
    """{(dtype name, N): (sha256 of dqkv, largest dqkv error / bar)} for N = 49 .. 256 in this process' wave count"""
    res = {}
    for dt in ac.DTYPES:
        ratios, digests = [], []
        for N in WAVE_NS:
            qkv, dout = _dev_inputs(N, dt)
            got = _fwd_bwd(qkv, dout)
            ratios.append(_ratios(got, ac.reference(qkv, dout), qkv, dout, dt)[2:].max())
            digests.append(hashlib.sha256(_bits(got[2]).cpu().numpy().tobytes()).hexdigest()[:20])
        for N, d, r in zip(WAVE_NS, digests, torch.stack(ratios).cpu().tolist()):
            res[(ac.dtype_name(dt), N)] = (d, r)
    return res


def _four_wave_worker(q):
    import os
    os.environ["SMOE_ATTN_BWD_WAVES"] = "4"            # read once per process, at the first backward (csrc/attention_bwd.hip)
    q.put(_bwd_digests())


def test_four_wave_backward_at_every_length_that_branches_on_the_wave_count():
    """<8,4>, <13,4>, <16,4> (and <4,4> at N = 49 .. 64) in a child process started with SMOE_ATTN_BWD_WAVES=4: dqkv inside the bars of
    (a) at every N, and -- what tests/test_gpu_dense.py pins at six shapes -- the same bits as the 8-wave form of this process."""
    import queue
    import torch.multiprocessing as mp
    from _mp import join_or_kill
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_four_wave_worker, args=(q,))
    p.start()
    mine = _bwd_digests()                               # the parent's 8-wave values, while the child works
    four, deadline = None, time.time() + 240
    while four is None and time.time() < deadline:
        try:
            four = q.get(timeout=0.5)
        except queue.Empty:
            if not p.is_alive():
                break
    join_or_kill([p], 30)
    assert four is not None and set(four) == set(mine) and len(four) == 2 * len(WAVE_NS)
    for dtn in ("f16", "bf16"):
        w, N = max((four[(dtn, N)][1], N) for N in WAVE_NS)
        print(f"4-wave backward {dtn}: worst dqkv error / bar {w:.3f} at N {N}; "
              f"{sum(four[(dtn, N)][0] == mine[(dtn, N)][0] for N in WAVE_NS)} of {len(WAVE_NS)} lengths bit-identical to 8 waves")
    bad = [(k, round(v[1], 3)) for k, v in sorted(four.items()) if not v[1] <= 1.0]
    assert not bad, f"4-wave dqkv over the bar: {bad}"
    bad = [(k, round(v[1], 3)) for k, v in sorted(mine.items()) if not v[1] <= 1.0]
    assert not bad, f"8-wave dqkv over the bar: {bad}"
    differ = [k for k in sorted(four) if four[k][0] != mine[k][0]]
    assert not differ, f"4-wave and 8-wave dqkv differ in bits at {differ}"


# --------------------------------------------------------------------------------------------------------------- varlen sweep
@functools.lru_cache(maxsize=None)
def _varlen_setup(dt):
    """per batch: compact qkv [rows, 3, H, 64] with zero unowned rows, the plan on the device, the owned-row mask and the float64
    reference [rows, H, 64] (zero on unowned rows) -- computed once per dtype, shared by the flag settings, never modified"""
    out = []
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    for i, (lens, mults, rs, rows) in enumerate(ac.varlen_batches()):
        qkv = ac.varlen_inputs(i, rows, dt).to(DEV)
        owned = torch.zeros(rows, dtype=torch.bool, device=DEV)
        ref = torch.zeros(rows, ac.H, 64, dtype=torch.float64, device=DEV)
        for L, m, r in zip(lens, mults, rs):
            owned[r:r + L] = True
            ref[r:r + L] = ac.varlen_reference(qkv[r:r + L], m)
        qkv[~owned] = 0
        out.append(dict(qkv=qkv, owned=owned, ref=ref, lens=lens, mults=mults, rs=rs, rows=rows, plan=(i32(rs), i32(lens), i32(mults))))
    return out


def _varlen_call(qkv, batch, flags):
    """smoe_attention_fwd_varlen into a caller-owned, payload-filled buffer -> the int16 buffer (guards included)"""
    rows, dt = batch["rows"], qkv.dtype
    buf, ptr = _guarded(rows * ac.H * 64, dt)
    rs, ln, mu = batch["plan"]
    rc = _lib.load().smoe_attention_fwd_varlen(qkv.data_ptr(), ptr, ops.dtype_code(dt), rs.data_ptr(), ln.data_ptr(), mu.data_ptr(),
                                               len(batch["lens"]), max(batch["lens"]), rows, ac.H, 64, 0.125, int(flags),
                                               ops._stream(qkv))
    _lib.check(rc, "smoe_attention_fwd_varlen")
    return buf


# (tests/test_gpu_skip_attention.py runs the default flags only; the second setting here is the one that changes which
#  instantiation a LENGTH takes -- without tiers every image walks the batch's key-tile count.  Both weight the last key's
#  probability, which is what VARLEN_BAR was measured for.)
@pytest.mark.parametrize("flags", [0, ops.VARLEN_NO_TIERS], ids=["tiers", "no-tiers"])
@pytest.mark.parametrize("dt", ac.DTYPES, ids=ac.dtype_name)
def test_varlen_every_length_and_multiplicity(dt, flags):
    worst, bad = (-1.0, (0, 0)), []
    for bi, batch in enumerate(_varlen_setup(dt)):
        rows, owned = batch["rows"], batch["owned"]
        n = rows * ac.H * 64
        buf = _varlen_call(batch["qkv"], batch, flags)
        inner = buf[GUARD:GUARD + n].reshape(rows, ac.H, 64)
        payload = ac.NAN16[dt]
        if not (bool((buf[:GUARD] == payload).all()) and bool((buf[GUARD + n:] == payload).all())):
            bad.append((bi, "guard band written"))
        if not bool((inner[~owned] == payload).all()):
            bad.append((bi, "an unowned row was written"))
        err = (inner.view(dt).double() - batch["ref"]).abs().amax(dim=(1, 2))              # per row; NaN where never written
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)[owned]
        rows_owned = torch.nonzero(owned).flatten()
        e, at = err.max(dim=0)
        e, at = float(e), int(rows_owned[at])
        img = max(i for i, r in enumerate(batch["rs"]) if r <= at)
        worst = max(worst, (e, (batch["lens"][img], batch["mults"][img])))
        if not e <= VARLEN_BAR[dt]:
            over = {(batch["lens"][i], batch["mults"][i]) for i, r in enumerate(batch["rs"])
                    if not float(err[(rows_owned >= r) & (rows_owned < r + batch["lens"][i])].max()) <= VARLEN_BAR[dt]}
            bad.append((bi, "(len, mult) over the bar", sorted(over)))
        qn = batch["qkv"].clone()                                     # the unowned input rows: zeros -> NaN
        _bits(qn)[~owned] = payload
        again = _varlen_call(qn, batch, flags)
        if not torch.equal(again, buf):
            bad.append((bi, "NaN in unowned input rows changed the output's bits"))
    print(f"varlen sweep {ac.dtype_name(dt)} flags {flags}: max |out - float64| {worst[0]:.3e} at (len, mult) {worst[1]}; "
          f"bar {VARLEN_BAR[dt]:.3e}")
    assert not bad, f"{bad}"


# ------------------------------------------------------------------------------------------------------------ skip plan sweep
@pytest.mark.parametrize("park_cols", [0, 8], ids=["no-park", "park"])
def test_skip_plan_at_every_length(park_cols):
    """B = 3: an all-bypassed image, a none-bypassed one and a random one, N = 1 .. 256, against the host plan bit for bit."""
    bad = []
    for N in ac.VARLEN_LENS:
        byp = np.zeros((3, N), dtype=bool)
        byp[0] = True
        byp[2] = np.random.default_rng(N).random(N) < 0.5
        park = torch.full((3, park_cols), 7.0, device=DEV) if park_cols else None
        got = ops.skip_plan(sc.mask_from_bypass(byp).to(DEV), 3, N, park=park)
        for k, w in sc.host_plan(byp).items():
            if not np.array_equal(got[k].cpu().numpy(), w):
                bad.append((N, k))
        if park is not None and float(park.abs().max()) != 0.0:
            bad.append((N, "park not zeroed"))
    assert not bad, f"{bad}"
