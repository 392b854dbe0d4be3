"""The gates of the MoE operator (fmoe.gates: NaiveGate, SwitchGate, GShardGate, NoisyGate) and the one no-grad routing sequence.

What a gate adds around the HIP router call is stated HERE, once per class: the routing sites (fmoe.FMoETransformerMLP,
ep.ep_forward_steps, autograd._route_train) never ask which class a gate is.  The surface is _GateBase's; DESIGN.md lists it."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from . import ops
from ._cache import StreamCache, param_version


class Routed:
    """What one routing pass hands its site: the router's ``idx`` / ``score`` / ``probs`` (/ ``logits`` in training), ``src`` = the rows
    the experts' operand is gathered from (x, or the LayerNorm's 16-bit image), what the dispatch plan runs over (``plan_idx``,
    ``plan_cap``) and with (``hist``), and ``state`` = what the gate's own forward step keeps for its score."""
    __slots__ = ("idx", "score", "probs", "logits", "src", "plan_idx", "plan_cap", "hist", "state")


def route_nograd(mod, x: torch.Tensor, norm: Optional[nn.LayerNorm] = None, cd: Optional[torch.dtype] = None, sub=None,
                 want_hist: bool = True) -> Routed:
    """The no-grad routing sequence of every site: operands, noise, the router call -- plain, or LayerNorm + router in one pass
    with ``norm`` (``src`` is then the normalised image in ``cd``) -- or the detour of a NoisyGate left in training mode, then the
    plan input.  ``sub`` (a row subset the plan will cover) / ``want_hist`` False: no chunk histogram, it counts every row."""
    g, k = mod.gate, mod.top_k
    T, d = x.shape
    r = Routed()
    r.src, r.hist = x, None
    if not g.fused_pass_ok():     # a no-grad forward of a module left in training mode routes with noise
        assert norm is None, "route_nograd: a NoisyGate in training mode takes the unfused sequence"
        (r.idx, r.score), r.probs = g.route_noisy(x), None
    else:
        wg, bg = g.router_operands()
        noise = g.router_noise(T, x.device)
        if norm is not None:
            # the router pass also counts for the plan (count_by_gate folded in) -- over all rows: of no use to a plan over some,
            # nor to one over ids the gate prunes behind the router
            if want_hist and sub is None and not g.prunes:
                r.hist = ops.chunk_hist(T, d, g.tot_expert, k, x.device)
            r.src, _, r.idx, r.score, _, r.probs = ops.ln_router_topk(
                x, norm.weight.detach().float(), norm.bias.detach().float() if norm.bias is not None else None, norm.eps,
                wg, bg, k, g.kind, noise, xn16_dtype=cd, want_probs=g.want_probs, hist=r.hist)
        else:
            r.idx, r.score, _, r.probs = ops.router_topk(x, wg, bg, k, g.kind, noise, want_probs=g.want_probs)
    r.plan_idx, r.plan_cap = g.plan_input(r.idx, r.score, T)
    return r


class _ScoreAux(torch.autograd.Function):
    """A gate's differentiable ``(score, aux)`` from what the HIP kernels already computed, as ONE node back to the logits: the
    forward hands both through; the backward is the gate's own one-pass kernel ``bwd(dscore f32 | None, scale f32 [1] | None,
    *saved) -> dlogits`` (``scale`` = the loss' gradient, multiplied onto the loss coefficients inside the kernel; None = no aux
    loss in the objective: its terms are left out)."""

    @staticmethod
    def forward(ctx, logits, score, aux, bwd, *saved):
        ctx.bwd = bwd
        ctx.save_for_backward(*saved)
        ctx.set_materialize_grads(False)     # no aux loss in the objective: daux is None, not a zero tensor
        return score.view_as(score), aux.view_as(aux)

    @staticmethod
    def backward(ctx, dscore, daux):
        saved = ctx.saved_tensors
        if dscore is None and daux is None:
            return (None,) * (4 + len(saved))
        ds = dscore.to(torch.float32).contiguous() if dscore is not None else None
        scale = daux.reshape(1).to(torch.float32) if daux is not None else None
        return (ctx.bwd(ds, scale, *saved),) + (None,) * (3 + len(saved))


class _GateBase(nn.Module):
    """What every gate holds (fmoe.gates.BaseGate) and the per-gate surface with the answers of a gate that adds nothing."""

    kind = ops.GATE_NAIVE
    want_probs = False        # the router also stores softmax(logits + noise) [T, E]
    prunes = False            # the plan runs over ids the gate prunes behind the router (plan_input): the router's chunk histogram
    #                           does not describe them, and a pre-routed batch's own plan ids would be lost
    zero_groups_ok = False    # all-zero rows route alike and may get row groups of their own (autograd._route_train)

    def __init__(self, num_expert: int, world_size: int, top_k: int):
        super().__init__()
        self.top_k = top_k
        self.num_expert, self.world_size = num_expert, world_size
        self.tot_expert = num_expert * world_size
        self.loss = None

    def capacity(self, n_tokens: int) -> int:
        return -1

    def rate(self) -> Optional[float]:
        """``capacity_factor`` as one rate: of a (train, eval) pair the one of the module's mode."""
        cf = self.capacity_factor
        if isinstance(cf, (tuple, list)):
            cf = cf[0] if self.training else cf[1]
        return cf

    def set_loss(self, loss):
        self.loss = loss

    def get_loss(self, clear: bool = True):
        loss = self.loss
        if clear:
            self.loss = None
        return loss

    def skip_gate_fusable(self) -> bool:
        """Whether the token-skip gate's fused pass (ops.gate_ln_router), which routes by the NaiveGate's rule, routes for this gate."""
        return False

    # -- the router call ---------------------------------------------------------------------------------------------
    def router_operands(self):
        """(wg f32 [E, d] contiguous, bg f32 [E] | None) without a gradient, read from ``self.gate`` as it is now."""
        lin = self.gate
        return lin.weight.detach().float().contiguous(), lin.bias.detach().float() if lin.bias is not None else None

    def router_noise(self, T: int, device) -> Optional[torch.Tensor]:
        return None

    # -- a no-grad forward -------------------------------------------------------------------------------------------
    def fused_pass_ok(self) -> bool:
        """Whether the plain / LayerNorm-fused router pass routes for this gate now."""
        return True

    def plan_input(self, idx: torch.Tensor, score: torch.Tensor, T: int):
        """(ids, capacity) the dispatch plan runs over."""
        return idx, self.capacity(T)

    def nograd_loss(self, kept: Optional[torch.Tensor], probs: Optional[torch.Tensor]) -> None:
        """The loss a no-grad forward leaves: ``kept`` = the ids the plan kept (None on a rank that planned nothing)."""

    # -- a training forward ------------------------------------------------------------------------------------------
    score_grad = property(lambda self: self.top_k > 1)    # (top-1 naive: softmax over one logit == 1, no gradient)

    def train_begin(self, T: int, device):
        """(gate weight, bias -- as autograd sees them --, the router call's k, its noise, the gate's own draw)."""
        return self.gate.weight, self.gate.bias, self.top_k, self.router_noise(T, device), None

    def train_torch(self, x: torch.Tensor, draw):
        """(idx, score) as differentiable torch ops where the kernels do not take this gate's configuration, else None."""
        return None

    def train_step(self, r: Routed, T: int):
        """The gate's own forward step behind the router call (no grad): may replace ``idx`` / ``score`` on the record and keep what
        ``train_score`` needs in ``r.state``; returns the plan input."""
        return self.plan_input(r.idx, r.score, T)

    def train_score(self, logits: torch.Tensor, r: Routed, counts: torch.Tensor) -> torch.Tensor:
        """The differentiable score from the logits node; sets the loss where the gate has one."""
        return torch.softmax(logits.gather(1, r.idx), dim=-1)

    def _score_aux(self, logits, score, aux, bwd, *saved) -> torch.Tensor:
        score, aux = _ScoreAux.apply(logits, score, aux, bwd, *saved)
        self.set_loss(aux)
        return score


class NaiveGate(_GateBase):
    """``gate = nn.Linear(d_model, num_expert * world_size)``; top-k of the logits, softmax over the kept k."""

    zero_groups_ok = True

    def __init__(self, d_model: int, num_expert: int, world_size: int, top_k: int = 2):
        super().__init__(num_expert, world_size, top_k)
        self.gate = nn.Linear(d_model, num_expert * world_size)

    def skip_gate_fusable(self) -> bool:
        return type(self) is NaiveGate      # (this very rule, not a subclass')


def switch_aux_loss(idx_pruned: torch.Tensor, probs: torch.Tensor, E: int) -> torch.Tensor:
    """aux = E * sum_e frac_e * prob_e: frac_e = share of kept tokens routed to e,
    prob_e = sum_t p[t,e] / kept.  Small [E]-sized reduction; differentiable w.r.t. ``probs``."""
    flat = idx_pruned.reshape(-1)
    keep = flat >= 0
    kept = keep.sum().clamp(min=1).to(probs.dtype)
    frac = torch.bincount(torch.where(keep, flat, torch.zeros_like(flat)), weights=keep.to(probs.dtype),
                          minlength=E)[:E] / kept
    prob = probs.sum(0) / kept
    return E * (frac * prob).sum()


class SwitchGate(NaiveGate):
    """Switch-Transformer top-1 gate with capacity and load-balance loss (fmoe.gates.SwitchGate).

    ``capacity_factor`` follows the Switch definition per source rank: cap = ceil(cf * T_local * k / E_total);
    ``capacity_mode="fmoe"`` selects upstream's ceil(cf * T_local) instead (cf = (train, eval) pair)."""

    kind = ops.GATE_SWITCH
    want_probs = True
    zero_groups_ok = False
    score_grad = True

    def __init__(self, d_model: int, num_expert: int, world_size: int, top_k: int = 1, switch_eps: float = 0.1,
                 capacity=(1.2, 2.4), capacity_mode: str = "switch"):
        assert top_k == 1, "SwitchGate is top-1"
        super().__init__(d_model, num_expert, world_size, top_k=1)
        self.switch_eps = switch_eps
        self.capacity_factor = capacity
        self.capacity_mode = capacity_mode

    def capacity(self, n_tokens: int) -> int:
        cf = self.rate()
        if cf is None:
            return -1
        if self.capacity_mode == "fmoe":
            return int(math.ceil(cf * n_tokens))
        return int(math.ceil(cf * n_tokens * self.top_k / self.tot_expert))

    def make_noise(self, T: int, device) -> Optional[torch.Tensor]:
        if not self.training or self.switch_eps <= 0:
            return None
        # upstream adds U[0,1) * 2*eps + (1 - eps) to the logits: one generator kernel (uniform_ applies the affine map itself)
        return torch.empty(T, self.tot_expert, device=device).uniform_(1.0 - self.switch_eps, 1.0 + self.switch_eps)

    def router_noise(self, T: int, device) -> Optional[torch.Tensor]:
        return self.make_noise(T, device)

    def nograd_loss(self, kept, probs) -> None:
        if kept is not None:
            self.set_loss(switch_aux_loss(kept, probs, self.tot_expert))

    def train_score(self, logits, r, counts):
        """score = softmax(logits + noise)[idx] and the load-balance loss aux = E sum_e frac_e prob_e from the router's own
        probabilities and score; backward ONE pass over [T, E] (smoe_switch_gate_bwd) instead of the ~25 small autograd kernels of
        softmax / gather / bincount / where."""
        # aux and cbase[e] = E frac_e / kept = d aux / d p[t, e] (the same for every t; dropped tokens count nowhere): smoe_switch_aux
        aux, cbase = ops.switch_aux(r.probs, counts)
        return self._score_aux(logits, r.score, aux, self._score_bwd, r.probs, r.idx, cbase)

    @staticmethod
    def _score_bwd(ds, scale, probs, idx, cbase):
        return ops.switch_gate_bwd(probs, idx.reshape(-1), ds.reshape(-1) if ds is not None else None,
                                   cbase if scale is not None else None, scale)


class GShardGate(NaiveGate):
    """GShard top-2 gate with a per-expert capacity, the GShard balance loss and random routing of the second choice
    (fmoe.gates.GShardGate; the rule is restated in INTEGRATION.md).  The routing is the naive top-2 router's; this gate's own
    arithmetic runs behind it on smoe_gshard_prune / _aux / _gate_bwd.

    ``capacity`` = (train, eval) rates or one rate for both: cap = (ceil(rate * T_local) * 2) // E_total entries per expert, applied
    per source rank in flat order (entry 2 t + j).  ``random_routing``: the second choice of token t is dropped when
    2 * score[t, 1] < u[t], u ~ U[0, 1) -- in training AND in eval, as upstream; pass False for a deterministic gate."""

    prunes = True
    zero_groups_ok = False    # (even without a capacity: random routing still drops entries)

    def __init__(self, d_model: int, num_expert: int, world_size: int, topk: int = 2, capacity=(1.2, 2.4),
                 random_routing: bool = True, gate_bias: bool = True):
        assert topk == 2, "GShardGate is top-2"
        super().__init__(d_model, num_expert, world_size, top_k=2)
        if not gate_bias:
            self.gate = nn.Linear(d_model, self.tot_expert, bias=False)
        self.capacity_factor = capacity
        self.random_routing = random_routing
        self.last_routing = None  # (u | None, idx_out, top1_counts) of the latest forward, for inspection

    def capacity(self, n_tokens: int) -> int:
        cf = self.rate()
        if cf is None:
            return -1
        return (int(math.ceil(cf * n_tokens)) * self.top_k) // self.tot_expert

    def make_uniform(self, T: int, device) -> Optional[torch.Tensor]:
        return torch.rand(T, device=device) if self.random_routing else None

    def prune(self, idx: torch.Tensor, score: torch.Tensor):
        """(idx_out, top1_counts) for the router's ``idx`` / ``score`` [T, 2]: capacity, then random routing (ops.gshard_prune).  The
        dispatch plan then runs over ``idx_out`` without a capacity of its own."""
        T = idx.shape[0]
        u = self.make_uniform(T, idx.device)
        idx_out, top1 = ops.gshard_prune(idx, score, u, self.tot_expert, self.capacity(T))
        self.last_routing = (u, idx_out, top1)
        return idx_out, top1

    def plan_input(self, idx, score, T):
        # capacity (per source rank, on this rank's T rows) + random routing on the gate's own kernels: every plan runs over what
        # is left, without a capacity of its own
        return (self.prune(idx, score)[0] if T > 0 else idx), -1

    def train_step(self, r, T):
        idx_out, r.state = self.prune(r.idx, r.score)      # (state: the first choices' counts, what train_score's loss is made of)
        return idx_out, -1

    def nograd_loss(self, kept, probs) -> None:
        self.set_loss(None)     # (no balance loss in a no-grad forward: nothing reads it, and it would cost a logits store)

    def train_score(self, logits, r, counts):
        """score = the router's softmax over the two chosen logits and aux = mean_e(c_e m_e) num_expert^2 from the logits and the
        first choices (smoe_gshard_aux); backward ONE pass over [T, E] (smoe_gshard_gate_bwd): the score gradient of an entry the
        prune dropped counts as zero."""
        aux, coef = ops.gshard_aux(logits.detach(), r.state, self.num_expert)
        return self._score_aux(logits, r.score, aux, self._score_bwd, logits, r.score, r.idx, r.plan_idx, coef)

    @staticmethod
    def _score_bwd(ds, scale, logits, score, idx, idx_out, coef):
        return ops.gshard_gate_bwd(logits, idx, idx_out, score, ds, coef if scale is not None else None, scale)


class _GateImage:
    """What the naive paths read as ``gate.gate`` of a NoisyGate: ``weight`` = the [E, d] f32 image of ``w_gate`` (no gradient), no bias."""
    __slots__ = ("weight", "bias")

    def __init__(self, weight):
        self.weight, self.bias = weight, None


class NoisyGate(_GateBase):
    """Noisy top-k gate with the importance + load balance loss and no capacity (fmoe.gates.NoisyGate, Shazeer et al.; the rule is
    restated in INTEGRATION.md).  Parameters ``w_gate`` / ``w_noise`` [d_model, E], no bias.  In training the router runs over the
    [2E, d] image [w_gate^T ; w_noise^T] and the gate's own arithmetic runs behind it on smoe_noisy_gate_fwd / _bwd; in eval
    (sigma = 0) the gate IS a bias-free NaiveGate over ``w_gate.T``: ``gate.gate`` hands every naive path that [E, d] image (cached
    per parameter version; not a sub-module, so the state dict holds ``w_gate`` and ``w_noise`` and nothing else).
    Calling the module (``gate(x)`` -> (idx, score)) is the differentiable torch composition of the rule: CPU tensors, and the
    configurations the kernels do not take."""

    score_grad = True

    def __init__(self, d_model: int, num_expert: int, world_size: int, top_k: int = 2):
        super().__init__(num_expert, world_size, top_k)
        if not 1 <= top_k < self.tot_expert:
            # (upstream falls back to a count-based, non-differentiable load at top_k >= E: refused instead)
            raise ValueError(f"NoisyGate: top_k={top_k} must be in [1, E) for E={self.tot_expert} experts (the load reads the "
                             f"(k+1)-th value)")
        self.w_gate = nn.Parameter(torch.empty(d_model, self.tot_expert))
        self.w_noise = nn.Parameter(torch.empty(d_model, self.tot_expert))
        self.noise_epsilon = 1e-2
        self.last_noise = None   # (eps, imp, load) of the latest training forward, for inspection
        self._images = StreamCache()
        self.register_load_state_dict_post_hook(lambda mod, _keys: mod._images.invalidate())
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.w_gate, a=math.sqrt(5))
        nn.init.kaiming_uniform_(self.w_noise, a=math.sqrt(5))

    def make_noise(self, T: int, device) -> torch.Tensor:
        return torch.randn(T, self.tot_expert, device=device)

    @property
    def gate(self) -> _GateImage:
        w = self.w_gate
        return _GateImage(self._images.get(("t", w.device), param_version(w), lambda: w.detach().t().float().contiguous()))

    def weight2(self) -> torch.Tensor:
        """[2E, d] = [w_gate^T ; w_noise^T], differentiable: the operand of the one router call that yields clean and raw logits."""
        return torch.cat((self.w_gate.t(), self.w_noise.t()), 0).float()

    def image2(self) -> torch.Tensor:
        """``weight2()`` without a gradient, cached per version of the two parameters."""
        ver = (param_version(self.w_gate), param_version(self.w_noise))
        return self._images.get(("2", self.w_gate.device), ver, lambda: self.weight2().detach().contiguous())

    def fused_pass_ok(self) -> bool:
        return not self.training      # (eval: sigma = 0, the gate is the bias-free NaiveGate over w_gate.T)

    def nograd_loss(self, kept, probs) -> None:
        self.set_loss(None)

    def route_noisy(self, x: torch.Tensor):
        """(idx, score) of a no-grad forward of a gate left in training mode: router over the [2E, d] image (its own top-1 is
        discarded), then smoe_noisy_gate_fwd with a fresh draw.  No loss."""
        T, E, k = x.shape[0], self.tot_expert, self.top_k
        self.set_loss(None)
        with torch.no_grad():
            if not ops.noisy_gate_supported(E, k):
                return self.forward(x.float())
            _, _, logits2, _ = ops.router_topk(x, self.image2(), None, 1, ops.GATE_NAIVE, None, want_logits=True)
            eps = self.make_noise(T, x.device)
            r = ops.noisy_gate_fwd(logits2, eps, k, True)
            self.last_noise = (eps, r["imp"], r["load"])
        return r["idx"], r["score"]

    def train_begin(self, T, device):
        # the gate "linear" is the [2E, d] stack [w_gate^T ; w_noise^T], built differentiably from the two parameters: ONE router call
        # (k = 1: its own top-1 over the 2E columns is discarded, the decision is taken on the f32 noisy values) yields clean and
        # raw logits, and its gradients go back through the same nodes as any gate's
        return self.weight2(), None, 1, None, (self.make_noise(T, device) if self.training else None)    # (eval: sigma = 0)

    def train_torch(self, x, draw):
        return None if ops.noisy_gate_supported(self.tot_expert, self.top_k) else self(x.float(), draw)

    def train_step(self, r, T):
        eps = r.state
        nz = ops.noisy_gate_fwd(r.logits, eps, self.top_k, self.training)
        r.idx, r.score, r.state = nz["idx"], nz["score"], (eps, nz)
        self.last_noise = (eps, nz["imp"], nz["load"])
        return r.idx, -1

    def train_score(self, logits, r, counts):
        """score = softmax over the k largest noisy values and aux = cv2(importance) + cv2(load) are smoe_noisy_gate_fwd's own;
        ``logits`` [T, 2E] = [clean | raw] carries the gradient, backward ONE pass (smoe_noisy_gate_bwd)."""
        (eps, nz), training = r.state, self.training
        return self._score_aux(
            logits, r.score, nz["aux"],
            lambda ds, scale, lg, eps, idx, keep, nxt, ci, cl: ops.noisy_gate_bwd(lg, eps, idx, keep, nxt, ds, ci, cl, scale, training),
            logits, eps, r.idx, nz["keep"], nz["next"], nz["coef_imp"], nz["coef_load"])

    @staticmethod
    def cv2(v: torch.Tensor) -> torch.Tensor:
        return v.var(unbiased=True) / (v.mean() ** 2 + 1e-10)

    def forward(self, inp: torch.Tensor, eps: Optional[torch.Tensor] = None):
        """(idx int64 [T, k], score [T, k]) by the rule as differentiable torch ops; sets the loss (None without grad)."""
        E, k = self.tot_expert, self.top_k
        x = inp.reshape(-1, inp.shape[-1])
        clean = x @ self.w_gate.to(x.dtype)
        if self.training:
            sigma = torch.nn.functional.softplus(x @ self.w_noise.to(x.dtype)) + self.noise_epsilon
            if eps is None:
                eps = self.make_noise(x.shape[0], x.device)
            noisy = clean + eps.to(x.dtype) * sigma
        else:
            noisy = clean
        val, order = torch.sort(noisy, dim=1, descending=True, stable=True)      # (stable: ties -> lowest expert id)
        idx, v = order[:, :k], val[:, :k + 1]
        score = torch.softmax(v[:, :k], dim=-1)
        if not (torch.is_grad_enabled() and (x.requires_grad or self.w_gate.requires_grad or self.w_noise.requires_grad)):
            self.set_loss(None)
            return idx, score
        imp = torch.zeros(E, dtype=score.dtype, device=x.device).scatter_add(0, idx.reshape(-1), score.reshape(-1))
        aux = self.cv2(imp)
        if self.training:
            thr = torch.where(noisy > v[:, k:k + 1], v[:, k:k + 1], v[:, k - 1:k])
            load = (0.5 * (1.0 + torch.erf((clean - thr) / sigma * (1.0 / math.sqrt(2.0))))).sum(0)
            aux = aux + self.cv2(load)
        self.set_loss(aux)
        return idx, score
