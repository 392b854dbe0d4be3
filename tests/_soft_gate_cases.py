"""The soft token-skip gate (Gate(is_hard=False) in training; csrc/soft_gate.hip, gate_on = 2 of the two gate backward kernels):
float64 references, an f32 emulation of the forward kernel's arithmetic and THE error bars, shared by tests/test_soft_gate_host.py
(which checks emulation and bars on the CPU) and tests/test_gpu_soft_gate.py (which holds the kernels to the same bars).

The bars are first-order rounding analysis in units of u = 2^-24 (half an f32 ulp), stated per quantity:

  xn      the LayerNorm bar of tests/test_value_regimes_host.py (ln_row_bar / ln_elem_bar; 0 without a LayerNorm: xn = x exactly)
  z       rowbar(xn) |w|_1  +  24 u sum_c |xn_c w_c|  +  u |z|       a lane adds at most 16 products by FMA, 6 butterfly levels, the bias:
                                                                     at most 24 roundings on any path, each relative to a partial sum
                                                                     bounded by sum |xn w|; the last add's own rounding is u |z|
  p       RELATIVE  (1 - p) zbar + 5 u                               d ln p / dz = 1 - p;  expf within one ulp (2 u), 1 + e (u),
  1 - p   RELATIVE  p zbar + 5 u                                     the division (u), and e's error enters 1 / (1 + e) halved at most
  tk      |xn| p pbar + p xnbar + u |tk|                             one f32 multiply of the two; a 16-bit image adds its store's half
                                                                     ulp (2^-11 f16 / 2^-8 bf16 relative, 2^-25 absolute for f16)

`ratio` functions return the worst |got - ref| / bar.  1 - p taken from the ROUNDED p has an absolute error of up to u / 2 whatever
1 - p is: relative to 1 - p = 4.5e-5 (z = 10) that is 1e3 bars."""
import math

import torch

from test_value_regimes_host import EPS, U, _butterfly, _fma, _slabs, ln_f64, ln_row_bar, ln_elem_bar

Z_ROUNDINGS = 24
P_ROUNDINGS = 5
_STORE = {torch.float32: (0.0, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25), torch.bfloat16: (2.0 ** -8, 0.0)}


def _affine(d, gamma, beta):
    return (torch.ones(d) if gamma is None else gamma.float()), (torch.zeros(d) if beta is None else beta.float())


def soft_f64(x, gamma, beta, w, b, ln=True):
    """float64 forward of one soft gated half on f32 rows x [R, d]: dict(xn, z, p, om = 1 - p (as sigmoid(-z)), tk, lnref)"""
    d = x.shape[1]
    gm, bt = _affine(d, gamma, beta)
    lnref = ln_f64(x, gm, bt) if ln else None
    xn = lnref["y"] if ln else x.double()
    z = xn @ w.double() + (0.0 if b is None else b.double())
    p, om = torch.sigmoid(z), torch.sigmoid(-z)
    return dict(xn=xn, z=z, p=p, om=om, tk=xn * p[:, None], lnref=lnref, gamma=gm)


def soft_bars(ref, w):
    """dict(xn_row [R], z [R], p_rel [R], om_rel [R]) for a soft_f64 result"""
    R = ref["xn"].shape[0]
    rb = ln_row_bar(ref["lnref"], ref["gamma"]) if ref["lnref"] is not None else torch.zeros(R, dtype=torch.float64)
    wd = w.double()
    zbar = rb * float(wd.abs().sum()) + Z_ROUNDINGS * U * (ref["xn"].abs() * wd.abs()).sum(-1) + U * ref["z"].abs()
    return dict(xn_row=rb, z=zbar, p_rel=ref["om"] * zbar + P_ROUNDINGS * U, om_rel=ref["p"] * zbar + P_ROUNDINGS * U)


def _worst(err, bar):
    r = err / bar
    r = torch.where(torch.isfinite(err), r, torch.full_like(r, math.inf))
    return float(r.max())


def soft_ratios(got, ref, w, dt16=None):
    """Worst error / bar of each output of the soft forward present in ``got`` (xn32, mask [R, 2] = (1 - p, p), tk32, xn16 = the
    16-bit image of tk in ``dt16``): dict name -> ratio."""
    bars = soft_bars(ref, w)
    out = {}
    g = {k: v.detach().double().cpu() for k, v in got.items() if v is not None}
    if ref["lnref"] is not None:
        xn_bar = ln_elem_bar(ref["lnref"], ref["gamma"])
    else:
        xn_bar = torch.full_like(ref["xn"], 1e-300)          # (without a LayerNorm xn32 is x, bit for bit)
    if "xn32" in g:
        out["xn32"] = _worst((g["xn32"] - ref["xn"]).abs(), xn_bar)
    if "mask" in g:
        out["p"] = _worst((g["mask"][:, 1] - ref["p"]).abs(), bars["p_rel"] * ref["p"])
        out["1-p"] = _worst((g["mask"][:, 0] - ref["om"]).abs(), bars["om_rel"] * ref["om"])
    p = ref["p"][:, None]
    tk_bar = ref["xn"].abs() * p * bars["p_rel"][:, None] + p * xn_bar + U * ref["tk"].abs() + 1e-300
    if "tk32" in g:
        out["tk32"] = _worst((g["tk32"] - ref["tk"]).abs(), tk_bar)
    if "xn16" in g:
        rel, ab = _STORE[dt16]
        out["tk16"] = _worst((g["xn16"] - ref["tk"]).abs(), tk_bar + rel * (ref["tk"].abs() + tk_bar) + ab)
    return out


def soft_emulate(x, gamma, beta, w, b, ln=True, subtract=False):
    """f32 emulation of soft_gate_ln_fwd_kernel: lane l holds elements [4 l + 256 j, + 4); mean from (x0 + x1) + (x2 + x3) per slab,
    the squares by FMA, both over the butterfly; xn = fma((x - mean) rstd, gamma, beta); the logit by FMA per lane and the butterfly;
    e = exp(-|z|), p and 1 - p as 1 / (1 + e) and e / (1 + e) by the sign of z -- or, ``subtract``, 1 - p from the rounded p, the form
    the kernel must NOT take; tk = xn p.  Returns dict(xn32, mask, tk32)."""
    R, d = x.shape
    gm_, bt_ = _affine(d, gamma, beta)
    xv, valid = _slabs(x.float(), 4)
    gm, _ = _slabs(gm_[None, :], 4)
    bt, _ = _slabs(bt_[None, :], 4)
    wv, _ = _slabs(w.float()[None, :], 4)
    if ln:
        inv_d = torch.tensor(1.0 / d, dtype=torch.float32)
        s1 = torch.zeros(R, 64)
        for j in range(xv.shape[1]):
            s1 = s1 + ((xv[:, j, :, 0] + xv[:, j, :, 1]) + (xv[:, j, :, 2] + xv[:, j, :, 3]))
        mean = _butterfly(s1) * inv_d
        s2 = torch.zeros(R, 64)
        for j in range(xv.shape[1]):
            for i in range(4):
                dv = xv[:, j, :, i] - mean[:, None]
                s2 = torch.where(valid[j][None, :], _fma(dv, dv, s2), s2)
        rstd = torch.rsqrt(_butterfly(s2) * inv_d + torch.tensor(EPS, dtype=torch.float32))
        xn = _fma((xv - mean[:, None, None, None]) * rstd[:, None, None, None], gm, bt)
        xn = torch.where(valid[None, :, :, None], xn, torch.zeros(()))
    else:
        xn = xv
    az = torch.zeros(R, 64)
    for j in range(xv.shape[1]):
        for i in range(4):
            az = _fma(xn[:, j, :, i], wv[:, j, :, i], az)
    z = _butterfly(az) + (torch.zeros(()) if b is None else b.float().reshape(()))
    e = torch.exp(-z.abs())
    den = 1 + e
    hi, lo = 1 / den, e / den
    pos = ~(z < 0)
    p = torch.where(pos, hi, lo)
    om = (1 - p) if subtract else torch.where(pos, lo, hi)
    xn = xn.reshape(R, -1)[:, :d]
    return dict(xn32=xn, mask=torch.stack((om, p), dim=1), tk32=xn * p[:, None])


def soft_bwd_f64(x, gamma, beta, w, b, g_f, g_out, ln=True):
    """float64 autograd through [LayerNorm and] the reference's SOFT gate expressions (models/resMoE.py:69-74, 126-136):
    skip_tk = 1 - p, tk = p, L = <g_f, xn tk> + <g_out, xn tk + xn skip_tk>.
    dict(dx, dgamma, dbeta, dgate_w, dgate_b, dz [R], dxn, xn, p, mask [R, 2] f32 = (1 - p, p))"""
    d = x.shape[1]
    gm, bt = _affine(d, gamma, beta)
    xr, gr, btr, wr = [t.double().requires_grad_(True) for t in (x, gm, bt, w)]
    br = (torch.zeros(1) if b is None else b).double().reshape(1).requires_grad_(True)
    xn = torch.nn.functional.layer_norm(xr, (d,), gr, btr, EPS) if ln else xr * 1.0
    xn.retain_grad()
    z = xn @ wr + br
    z.retain_grad()
    prob = torch.sigmoid(z)[:, None]
    skip_tk, tk = 1 - prob, prob
    loss = (g_f.double() * (xn * tk)).sum()
    if g_out is not None:
        loss = loss + (g_out.double() * (xn * tk + xn * skip_tk)).sum()
    loss.backward()
    zd = z.detach()
    mask = torch.stack((torch.sigmoid(-zd), torch.sigmoid(zd)), dim=1).float()
    return dict(dx=xr.grad, dgamma=gr.grad, dbeta=btr.grad, dgate_w=wr.grad, dgate_b=br.grad, dz=z.grad, dxn=xn.grad,
                xn=xn.detach(), p=prob.detach()[:, 0], mask=mask)


def saturating_rows(w, b, zs):
    """rows x [len(zs), d] f32 along w whose logit <x, w> + b is zs (to f32 rounding of x): the gate without a LayerNorm, saturated"""
    wd = w.double()
    bd = 0.0 if b is None else float(b)
    return ((torch.as_tensor(zs, dtype=torch.float64) - bd)[:, None] * wd[None, :] / float(wd @ wd)).float().contiguous()


def block_f64(P, x, heads, dense_soft, moe_soft, thr=0.6):
    """float64 copy of resmoe._residual_block_composed (models/resMoE.py:126-145) on the parameters ``P`` of ref_resblock_tiny.npz
    (name -> float64 leaf tensor; the dense Mlp is the E = 1 MoE), in TRAIN mode, each gate soft or hard (hard: decision p > thr,
    straight-through estimator).  Returns (y, (dense mask, moe mask), (dense logit, moe logit)), masks [B, N, 2] detached, the
    logits with retain_grad() (their gradient is dz)."""
    F = torch.nn.functional
    B, N, d = x.shape
    hd = d // heads

    def gated(xn, name, soft):
        z = F.linear(xn, P[name + ".head.1.weight"], P[name + ".head.1.bias"])
        z.retain_grad()
        p = torch.sigmoid(z)
        if soft:
            bypass, enter = 1 - p, p
        else:
            hard = (p > thr).double()
            st = p.detach() - p
            bypass, enter = hard - st, (1 - hard) + st
        return xn * enter, xn * bypass, torch.cat((bypass, enter), dim=-1).detach(), z

    xn = F.layer_norm(x, (d,), P["norm1.weight"], P["norm1.bias"], EPS)
    tk, sk, m1, z1 = gated(xn, "dense_gate", dense_soft)
    qkv = F.linear(tk, P["attn.qkv.weight"], P["attn.qkv.bias"]).reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    att = ((qkv[0] * hd ** -0.5) @ qkv[1].transpose(-2, -1)).softmax(dim=-1)
    a = F.linear((att @ qkv[2]).transpose(1, 2).reshape(B, N, d), P["attn.proj.weight"], P["attn.proj.bias"])
    x1 = a + tk + sk
    xn2 = F.layer_norm(x1, (d,), P["norm2.weight"], P["norm2.bias"], EPS)
    tk2, sk2, m2, z2 = gated(xn2, "moe_gate", moe_soft)
    h = F.gelu(F.linear(tk2, P["mlp.fc1.weight"], P["mlp.fc1.bias"]))
    return F.linear(h, P["mlp.fc2.weight"], P["mlp.fc2.bias"]) + tk2 + sk2, (m1, m2), (z1, z2)


def block_f64_grads(fixture, dense_soft, moe_soft, thr=0.6):
    """y, dx, parameter gradients (fixture names) and masks of block_f64 on a ref_resblock_tiny.npz dict with L = <dy, y>;
    dz_l1 = {gate name: sum_t |dz_t|}: a gate's bias gradient is the SUM of dz over the tokens, terms of both signs, so the scale of
    its rounding error is the sum of their magnitudes, not the magnitude of their sum"""
    P = {k[2:]: torch.from_numpy(v).double().requires_grad_(True) for k, v in fixture.items()
         if k.startswith("p.") and "threshold" not in k}
    x = torch.from_numpy(fixture["x"]).double().requires_grad_(True)
    y, masks, zs = block_f64(P, x, int(fixture["num_heads"]), dense_soft, moe_soft, thr)
    y.backward(torch.from_numpy(fixture["dy"]).double())
    return dict(y=y.detach(), dx=x.grad, g={k: v.grad for k, v in P.items()}, masks=masks,
                dz_l1={"dense_gate": float(zs[0].grad.abs().sum()), "moe_gate": float(zs[1].grad.abs().sum())})
