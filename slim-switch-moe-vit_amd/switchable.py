"""SwitchableLayerNorm and SwitchableVisionTransformer (models/layers.py:31-157, models/vision_transformer.py:325-640) with the
reference's attribute names and state-dict keys, the norm on the library's own kernels.

The rule (models/layers.py:105-151), per row of ``x [..., d]``::

    mean, biased var over d;  xhat = (x - mean) / sqrt(var + eps)
    bucket b = the given int / tensor entry, or argmin_k sum_j (x_j - c_kj)^2 over the RAW row (torch.argmin's rule)
    y = xhat * weights[b] + biases[b]

Upstream applies the affine with ``t[selected == i] = ...`` (boolean-mask indexing: two host synchronisations per bucket), which
no HIP graph can replay; here it is ONE launch forward (smoe_switch_ln_fwd) and four backward (smoe_switch_ln_bwd), so the model
runs under ``GraphedForward`` / ``GraphedTrainStep`` like the plain DeiT.  Deliberate differences:
``centroids`` start as zeros, not uninitialised memory; ``set_centroids`` takes a plain tensor; the selection is the exact argmin
of the direct form (upstream's f32 ``torch.cdist`` takes the expanded form and misassigns rows near a bisector)."""
from __future__ import annotations

import numbers
from collections import OrderedDict
from functools import partial
from typing import Optional

import torch
import torch.nn as nn

from .vit import (Block, DistilledVisionTransformer, PatchEmbed, VisionTransformer, _deit, _init_vit_weights, _warn_fallback,
                  register_model, trunc_normal_)

__all__ = ["SwitchableLayerNorm", "SwitchableVisionTransformer", "switch_ln_compose", "deit_sw_tiny_patch16_224"]


def switch_ln_compose(x: torch.Tensor, eps: float, weights: Optional[torch.Tensor], biases: Optional[torch.Tensor],
                      centroids: Optional[torch.Tensor], buckets=None, num_buckets: int = 1, ndims: int = 1):
    """The rule as a torch composition in ``x``'s dtype, differentiable, with ``weights[b]`` gathers instead of boolean masks (no
    host synchronisation).  The last ``ndims`` dims are normalised.  The distances are taken in float64 in the direct form: the
    selection is the exact one in every dtype.  ``buckets``: None, an int, or an integer tensor broadcasting to the leading dims.
    -> (y, buckets int64)."""
    lead = x.shape[: x.dim() - ndims]
    dims = tuple(range(-ndims, 0))
    mean = x.mean(dim=dims, keepdim=True)
    diff = x - mean
    var = diff.square().mean(dim=dims, keepdim=True)
    xhat = diff / torch.sqrt(var + eps)
    if buckets is None:
        if num_buckets == 1:
            b = torch.zeros(lead, dtype=torch.int64, device=x.device)
        else:
            rows = x.detach().reshape(lead + (-1,)).double()
            c = centroids.detach().reshape(num_buckets, -1).double()
            dist = torch.stack([(rows - c[k]).square().sum(-1) for k in range(num_buckets)], dim=-1)
            b = dist.argmin(dim=-1)
    elif isinstance(buckets, torch.Tensor):
        b = buckets.to(device=x.device, dtype=torch.int64).broadcast_to(lead)
    else:
        b = torch.full(lead, int(buckets), dtype=torch.int64, device=x.device)
    if weights is None:
        return xhat, b
    y = xhat * weights[b]
    if biases is not None:
        y = y + biases[b]
    return y, b


class _SwitchLNFn(torch.autograd.Function):
    """smoe_switch_ln_fwd / smoe_switch_ln_bwd.  x gets a gradient through the normalisation only, weights / biases the per-bucket
    sums (exact zeros for an empty bucket), centroids and the buckets none."""

    @staticmethod
    def forward(ctx, x, weights, biases, centroids, buckets, eps, K):
        from . import ops
        w = weights.detach() if weights is not None else None
        y, b = ops.switch_ln(x, w, biases.detach() if biases is not None else None,
                             centroids.detach() if (centroids is not None and buckets is None and K > 1) else None, eps, buckets,
                             num_buckets=K)
        ctx.eps, ctx.K = eps, K
        ctx.save_for_backward(x, w if w is not None else x.new_empty(0), b)
        ctx.mark_non_differentiable(b)
        return y, b

    @staticmethod
    def backward(ctx, dy, _db):
        from . import ops
        x, w, b = ctx.saved_tensors
        has_w = w.numel() > 0
        want = has_w and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dx, dw, dbias = ops.switch_ln_bwd(x, dy.contiguous(), w if has_w else None, b, ctx.eps, num_buckets=ctx.K,
                                          want_param_grads=want)
        return (dx if ctx.needs_input_grad[0] else None, dw if ctx.needs_input_grad[1] else None,
                dbias if ctx.needs_input_grad[2] else None, None, None, None, None)


class SwitchableLayerNorm(nn.Module):
    """models/layers.py:31-157: a LayerNorm with ``switchable_buckets`` affine pairs, one chosen per row -- by the caller
    (``buckets`` an int or an integer tensor: the curriculum stage) or by the nearest of ``centroids`` (``buckets=None``).
    ``forward(input, buckets=None) -> (out, buckets)``; ``input`` is not modified."""

    def __init__(self, normalized_shape, eps: float = 1e-5, elementwise_affine: bool = True, switchable_buckets: int = 1,
                 device=None, dtype=None) -> None:
        kw = {"device": device, "dtype": dtype}
        super().__init__()
        if isinstance(normalized_shape, numbers.Integral):
            normalized_shape = (int(normalized_shape),)
        self.normalized_shape = tuple(int(n) for n in normalized_shape)
        self.dims = tuple(i - len(self.normalized_shape) for i in range(len(self.normalized_shape)))
        self.eps = eps
        self.elementwise_affine = elementwise_affine
        self.switchable_buckets = int(switchable_buckets)
        if self.switchable_buckets < 1:
            raise ValueError("switchable_buckets must be >= 1")
        if elementwise_affine:
            self.weights = nn.Parameter(torch.empty((self.switchable_buckets, *self.normalized_shape), **kw))
            self.biases = nn.Parameter(torch.empty((self.switchable_buckets, *self.normalized_shape), **kw))
        else:
            self.register_parameter("weights", None)
            self.register_parameter("biases", None)
        numel = 1
        for n in self.normalized_shape:
            numel *= n
        # zeros (upstream: torch.empty, i.e. whatever the allocator hands out); in the state dict, never trained
        self.centroids = nn.Parameter(torch.zeros((self.switchable_buckets, numel), **kw), requires_grad=False)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        if self.elementwise_affine:
            nn.init.ones_(self.weights)
            nn.init.zeros_(self.biases)

    def set_centroids(self, centroids: torch.Tensor) -> None:
        """Replace the centroids ([switchable_buckets, prod(normalized_shape)]); a plain tensor or a Parameter."""
        if tuple(centroids.shape) != tuple(self.centroids.shape):
            raise ValueError(f"centroids must have shape {tuple(self.centroids.shape)}, got {tuple(centroids.shape)}")
        with torch.no_grad():
            self.centroids.copy_(centroids.detach().to(device=self.centroids.device, dtype=self.centroids.dtype))

    def _own_reason(self, x: torch.Tensor):
        """Why the kernels cannot take this call (None = they can)."""
        from . import ops
        if len(self.normalized_shape) != 1:
            return "tuple-valued normalized_shape"
        if x.dtype != torch.float32 or (self.weights is not None and self.weights.dtype != torch.float32) \
                or self.centroids.dtype != torch.float32:
            return "needs f32 rows and f32 tables"
        if not x.is_contiguous():
            return "rows not contiguous"
        if x.data_ptr() % 16 or any(t is not None and t.data_ptr() % 16 for t in (self.weights, self.biases, self.centroids)):
            return "rows or tables not 16-byte aligned"
        if not ops.switch_ln_supported(x.shape[-1], self.switchable_buckets):
            return f"d % 4 == 0, d <= 1024, buckets <= {ops.SWITCH_LN_MAX_BUCKETS}"
        return None

    def forward(self, input: torch.Tensor, buckets=None):
        K = self.switchable_buckets
        nd = len(self.normalized_shape)
        if tuple(input.shape[input.dim() - nd:]) != self.normalized_shape:
            raise RuntimeError(f"input {tuple(input.shape)} does not end in {self.normalized_shape}")
        lead = input.shape[: input.dim() - nd]
        if isinstance(buckets, bool) or (buckets is not None and not isinstance(buckets, (numbers.Integral, torch.Tensor))):
            raise TypeError("buckets: None, an int or an integer tensor")
        if isinstance(buckets, numbers.Integral):
            buckets = int(buckets)
            if not 0 <= buckets < K:
                raise ValueError(f"bucket {buckets} outside [0, {K})")
        elif isinstance(buckets, torch.Tensor):
            if torch.is_floating_point(buckets) or buckets.dtype == torch.bool:
                raise TypeError("a bucket tensor must have an integer dtype")
            capturing = input.is_cuda and torch.cuda.is_current_stream_capturing()
            if buckets.numel() and not capturing:     # upstream's range check (a host read: not while a graph is captured)
                lo, hi = int(buckets.min()), int(buckets.max())
                if lo < 0 or hi >= K:
                    raise ValueError(f"bucket tensor holds indices outside [0, {K})")
            buckets = buckets.to(device=input.device, dtype=torch.int64).broadcast_to(lead)
        if input.is_cuda:
            why = self._own_reason(input)
            if why is None:
                if isinstance(buckets, torch.Tensor):
                    buckets = buckets.contiguous()
                return _SwitchLNFn.apply(input, self.weights, self.biases, self.centroids, buckets, float(self.eps), K)
            _warn_fallback("switchable layer norm", why, input.shape)
        return switch_ln_compose(input, self.eps, self.weights, self.biases, self.centroids, buckets, K, nd)

    def extra_repr(self) -> str:
        return (f"{self.normalized_shape}, eps={self.eps}, elementwise_affine={self.elementwise_affine}, "
                f"switchable_buckets={self.switchable_buckets}")


class _BlockView:
    """``pre_blocks + mid_blocks + post_blocks`` read as one sequence: what ``VisionTransformer``'s helpers see as ``self.blocks``.
    Not a Module and not registered: the state-dict keys stay upstream's ``mid_blocks.N.*`` / ``post_blocks.N.*``."""

    def __init__(self, *seqs):
        self._seqs = seqs

    def __iter__(self):
        for s in self._seqs:
            yield from s

    def __len__(self):
        return sum(len(s) for s in self._seqs)

    def __getitem__(self, i):
        return list(self)[i]

    def __call__(self, x):
        for blk in self:
            x = blk(x)
        return x


class SwitchableVisionTransformer(VisionTransformer):
    """models/vision_transformer.py:325-640: a ViT whose token stream passes a ``SwitchableLayerNorm`` (``router``) between
    ``pre_blocks`` and ``mid_blocks``.  ``forward(x, bucket=None, threshold=None)`` -> logits, or ``(logits, embeddings)`` with
    ``collect_embeddings`` (the untouched pre-router stream); distilled: the pair of logits in training, their mean in eval.
    Embedding, blocks, final norm and heads run on ``VisionTransformer``'s paths.  ``routing = True`` is refused: upstream's branch
    (594-612) cannot execute, so there is no behaviour to match."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4.0, qkv_bias=True, representation_size=None, distilled=False, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.0, embed_layer=PatchEmbed, norm_layer=None, act_layer=None, weight_init="", buckets=1,
                 collect_embeddings=False):
        if weight_init != "":
            raise NotImplementedError("weight_init: only '' (the jax / nlhb schemes are not part of this build)")
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        act_layer = act_layer or nn.GELU
        super().__init__(img_size=img_size, patch_size=patch_size, in_chans=in_chans, num_classes=num_classes, embed_dim=embed_dim,
                         depth=0, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop_rate=drop_rate,
                         attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate, embed_layer=embed_layer,
                         norm_layer=norm_layer, act_layer=act_layer)
        del self.blocks                      # (empty: depth=0) -- `blocks` is the unregistered view below
        num_patches = self.patch_embed.num_patches
        if distilled:
            self.num_tokens = 2
            self.dist_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
            self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 2, embed_dim))
        self.router = SwitchableLayerNorm(embed_dim, switchable_buckets=buckets)
        self.router_start = 0
        self.router_end = -1
        self.routing = False
        self.collect_embeddings = collect_embeddings
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, depth)]

        def make(n, first):
            return nn.Sequential(*[
                Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate,
                      attn_drop=attn_drop_rate, drop_path=dpr[i + first], norm_layer=norm_layer, act_layer=act_layer,
                      num_tokens=num_patches + self.num_tokens) for i in range(n)])
        # upstream's counts and stochastic-depth indices (422-472), formula for formula: 0 / 11 / 1 blocks at depth 12
        self.pre_blocks = make(self.router_start % depth, 0)
        self.mid_blocks = make((self.router_end - self.router_start) % depth, self.router_start % depth)
        self.post_blocks = make((depth - self.router_end) % depth, self.router_end % depth)
        if representation_size and not distilled:
            self.num_features = representation_size
            self.pre_logits = nn.Sequential(OrderedDict([("fc", nn.Linear(embed_dim, representation_size)), ("act", nn.Tanh())]))
        self.head = nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()
        if distilled:
            self.head_dist = nn.Linear(self.embed_dim, self.num_classes) if num_classes > 0 else nn.Identity()
            trunc_normal_(self.dist_token, std=0.02)
        trunc_normal_(self.pos_embed, std=0.02)
        for m in (self.pre_blocks, self.mid_blocks, self.post_blocks, self.pre_logits, self.head, self.head_dist):
            if m is not None:
                m.apply(_init_vit_weights)

    @property
    def blocks(self):
        return _BlockView(self.pre_blocks, self.mid_blocks, self.post_blocks)

    def train(self, mode: bool = True):
        """Every child but ``router`` (models/vision_transformer.py:507-515)."""
        if not isinstance(mode, bool):
            raise ValueError("training mode is expected to be boolean")
        self.training = mode
        for name, module in self.named_children():
            if name != "router":
                module.train(mode)
        return self

    def route(self, mode: bool = True):
        self.routing = mode

    def get_classifier(self):
        return self.head if self.dist_token is None else (self.head, self.head_dist)

    def reset_classifier(self, num_classes, global_pool=""):
        self.num_classes = num_classes
        self.head = nn.Linear(self.embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        if self.num_tokens == 2:
            self.head_dist = nn.Linear(self.embed_dim, self.num_classes) if num_classes > 0 else nn.Identity()

    def forward_features(self, x, bucket=None, threshold=None):
        """-> (features, pre-router stream or None).  Features: [B, d], or the pair ([B, d], [B, d]) of a distilled model."""
        if self.routing:
            raise NotImplementedError("SwitchableVisionTransformer: routing=True is refused -- upstream's branch "
                                      "(models/vision_transformer.py:594-612) cannot execute, there is no behaviour to match")
        flag = bool(self.skip_aware_attention)
        for blk in self.blocks:
            if getattr(blk, "skip_aware_attention", False) != flag:
                blk.skip_aware_attention = flag
        x = self._embed(x)
        x = self.pre_blocks(x)
        pre_x = x if self.collect_embeddings else None
        x, bucket = self.router(x, bucket)
        after = list(self.mid_blocks) + list(self.post_blocks)
        if x.is_cuda and not torch.is_grad_enabled():    # (generator form: every block is handed the next block's norm1)
            from .ep import drain
            x = drain(self._blocks_steps(x, None, head_rows_only=True, blocks=after))
        else:
            for blk in after:
                x = blk(x)
        if self.dist_token is None:
            return self.pre_logits(self._final_norm_cls(x)), pre_x
        f = DistilledVisionTransformer._final_norm_cls(self, x)
        return (f[:, 0], f[:, 1]), pre_x

    def forward(self, x, bucket=None, threshold=None):
        f, embeddings = self.forward_features(x, bucket, threshold)
        if self.head_dist is not None:
            x, x_dist = self._head(self.head, f[0], "head_gemm"), self._head(self.head_dist, f[1], "head_dist_gemm")
            if self.training:
                return x, x_dist
            return (x + x_dist) / 2
        x = self._head(self.head, f, "head_gemm")
        return (x, embeddings) if self.collect_embeddings else x


@register_model
def deit_sw_tiny_patch16_224(pretrained=False, **kwargs):
    """models/model.py:103-122 (``buckets``, ``collect_embeddings``, ``depth`` ... pass through)."""
    return _deit(192, 12, 3, pretrained, cls=SwitchableVisionTransformer, **kwargs)
