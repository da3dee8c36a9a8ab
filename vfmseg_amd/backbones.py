"""ViT backbones + LoRA wrapper on the HIP kernels (reference: rein/models/backbones/{dino_v2,lora_backbone}.py).

The nn.Modules below are *parameter containers* that reproduce the reference's state_dict key scheme
 and registry names; the arithmetic lives in `DinoEngine`, which drives the C-ABI kernels:

  token layout  : rows [0, n*Np) = patch tokens (image-major), rows [n*Np, n*Np+n) = the [cls] tokens.  GEMM row
                  tiles therefore never straddle an odd 1025-token boundary and feature taps are plain row slices.
  residual      : fp32 [M, D]; GEMM operands in the compute dtype (bf16 | f32), fp32 accumulation.
  LoRA          : fused into the QKV projection by K-concatenation: [LN(x) | s*drop(LN(x)) A^T] @ [W | B]^T, so
                  the rank-32 path costs no extra pass over the activations (peft lora.Linear semantics,
                  lora_backbone.py:16-23; scaling alpha/r).  attn.proj, fc1 and fc2 take the same form when
                  Lora_config.target_modules names them (DinoEngine.sites()).
  backward      : hand-written (frozen base => only activation gradients + LoRA A/B weight gradients).
  full training : a bare DinoVisionTransformer in train() mode trains every base weight that enters the graph
                  (DinoEngine._backward_full: the weight / bias / LayerNorm / LayerScale / embedding gradients on top of the
                  activation gradients).
"""
import math

import os

import torch
import torch.nn as nn

from .precision import is_half
from . import ops
from .precision import compute_dtype
from .registry import MODELS

R_PAD = 64  # LoRA rank padded to one MFMA K-block

# Data-parallel overlap (vfmseg_amd.parallel): the backbone backward is the last and longest autograd node, so it tells
# the gradient synchroniser when buckets become final: "heads" when it starts (all decoder gradients are done) and
# "lora" (with the block index just finished) as it walks the blocks from the last to the first.
BACKWARD_EVENTS = {"heads_done": None, "block_done": None, "backbone_done": None}
# Backbone forward passes of the current step whose backward has not run yet.  Gradients shared by all layers (Rein) are final only when the
# LAST of them has run - a segmentor may send the backbone over two inputs per step - so "backbone_done" fires when this returns to zero.
_PENDING_BACKWARD = [0]


# ------------------------------------------------------------------------------------------ parameter containers
class _Lin(nn.Module):
    def __init__(self, i, o, bias=True):
        super().__init__()
        self.in_features, self.out_features = i, o
        self.weight = nn.Parameter(torch.empty(o, i))
        self.bias = nn.Parameter(torch.zeros(o)) if bias else None
        nn.init.trunc_normal_(self.weight, std=0.02)


class LoraLinear(nn.Module):
    """peft 0.10 lora.Linear key layout: base_layer.{weight,bias}, lora_A.default.weight, lora_B.default.weight."""

    def __init__(self, base, r, alpha, dropout):
        super().__init__()
        self.base_layer = base
        self.r, self.scaling, self.p = r, alpha / r, dropout
        a, b = _Lin(base.in_features, r, False), _Lin(r, base.out_features, False)
        nn.init.kaiming_uniform_(a.weight, a=math.sqrt(5))
        nn.init.zeros_(b.weight)
        self.lora_A = nn.ModuleDict({"default": a})
        self.lora_B = nn.ModuleDict({"default": b})


class _Attn(nn.Module):
    def __init__(self, dim, heads, qkv_bias, proj_bias):
        super().__init__()
        self.num_heads = heads
        self.qkv = _Lin(dim, dim * 3, qkv_bias)
        self.proj = _Lin(dim, dim, proj_bias)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden, bias):
        super().__init__()
        self.fc1 = _Lin(dim, hidden, bias)
        self.fc2 = _Lin(hidden, dim, bias)


class _LayerScale(nn.Module):
    def __init__(self, dim, init):
        super().__init__()
        self.gamma = nn.Parameter(init * torch.ones(dim))


class _Block(nn.Module):
    def __init__(self, dim, heads, mlp_ratio, qkv_bias, proj_bias, ffn_bias, init_values):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attn(dim, heads, qkv_bias, proj_bias)
        self.ls1 = _LayerScale(dim, init_values if init_values else 1.0)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio), ffn_bias)
        self.ls2 = _LayerScale(dim, init_values if init_values else 1.0)


class _PatchEmbed(nn.Module):
    def __init__(self, patch, in_chans, dim):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, dim, patch, patch)


@MODELS.register_module()
class DinoVisionTransformer(nn.Module):
    """Same ctor kwargs / state_dict keys as rein/models/backbones/dino_v2.py:55-182 (ffn_layer='mlp' only)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0,
                 qkv_bias=True, ffn_bias=True, proj_bias=True, drop_path_rate=0.0, drop_path_uniform=False,
                 init_values=None, ffn_layer="mlp", block_chunks=1, out_indices=(7, 11, 15, 23), init_cfg=None,
                 resize_feat=False, **kw):
        super().__init__()
        if ffn_layer != "mlp":
            raise NotImplementedError("only ffn_layer='mlp' (the reference's LoRA configs) is on the HIP path")
        if block_chunks not in (0, None):
            raise NotImplementedError("block_chunks must be 0 (all reference LoRA configs, lora_dinov2_ms_masked.py:27)")
        self.embed_dim = self.num_features = embed_dim
        self.patch_size, self.num_heads, self.n_blocks = patch_size, num_heads, depth
        self.out_indices = list(out_indices)
        self.img_size = img_size if isinstance(img_size, int) else img_size[0]
        self.patch_embed = _PatchEmbed(patch_size, in_chans, embed_dim)
        n = (self.img_size // patch_size) ** 2
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n + 1, embed_dim))
        self.blocks = nn.ModuleList(
            [_Block(embed_dim, num_heads, mlp_ratio, qkv_bias, proj_bias, ffn_bias, init_values) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)  # present in checkpoints, NOT applied to the taps (dino_v2.py:252-268)
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))
        self.drop_path_rate = float(drop_path_rate)
        self._full_train = False
        self._engine = None
        self.register_load_state_dict_post_hook(lambda m, keys: m.engine().invalidate())

    def inert_params(self):
        """Parameters of the checkpoint that never enter the graph: the final norm is not applied to the taps and nothing is masked."""
        return list(self.norm.parameters()) + [self.mask_token]

    def train(self, mode=True):
        """A bare backbone (no LoRA wrapper, no adapter) in train mode is fine-tuned whole.  torch's AdamW skips grad-less parameters, the
        flat-buffer optimiser would weight-decay them: `norm.*` and `mask_token` are frozen here (and stay in the checkpoint), as the inert
        EVA02 adapters are in LoRABackbone.train."""
        super().train(mode)
        self._full_train = bool(mode)
        if mode and self.engine().bare():
            for p in self.inert_params():
                p.requires_grad = False
        return self

    def full_training(self):
        """Is the base being trained?  (next to adapter_training(): what EncoderDecoder._tokens passes to forward_tokens)"""
        return self._full_train and self.engine().bare() and self.patch_embed.proj.weight.requires_grad

    def engine(self):
        if self._engine is None:
            self._engine = DinoEngine(self)
        return self._engine

    def forward_tokens(self, jobs, training=False, seed=None):
        """jobs: list of (img [B,3,H,W] fp32 cuda, box or None) that share one token grid. Returns Xcat
        [sum(B)*Np, 4*D] (compute dtype) - the four taps side by side, token-major - and (hp, wp)."""
        return _BackboneFn.apply(self, jobs, training, seed, *self.engine().trainable())

    def forward(self, x):
        xcat, (hp, wp) = self.forward_tokens([(x, None)], training=self.training and self.engine().lora_on())
        b, d = x.shape[0], self.embed_dim
        v = xcat.view(b, hp, wp, len(self.out_indices), d)
        return tuple(v[:, :, :, i].permute(0, 3, 1, 2) for i in range(len(self.out_indices)))  # NCHW-shaped views


@MODELS.register_module()
class Reins(nn.Module):
    """rein/models/backbones/reins.py:11-116: parameter container of the Rein adapter (same ctor kwargs, state_dict keys and initialisers).
    The arithmetic is DinoEngine's (`_rein_forward` / `_rein_backward`).  On the HIP path: softmax attention, a learnable `scale`, and no
    token-to-query link (the `rein_dinov2_linear.py` configs); `transform` / `merge` exist for the checkpoints' sake and never enter the graph."""

    def __init__(self, num_layers, embed_dims, patch_size, query_dims=256, token_length=100, use_softmax=True, link_token_to_query=True,
                 scale_init=0.001, zero_mlp_delta_f=False):
        super().__init__()
        if not use_softmax:
            raise NotImplementedError("Reins(use_softmax=False): the HIP adapter kernels compute the softmax form (all reference configs)")
        if zero_mlp_delta_f:
            raise NotImplementedError("Reins(zero_mlp_delta_f=True) replaces the learnable scale by the constant 1: not on the HIP path")
        if link_token_to_query:
            raise NotImplementedError("Reins(link_token_to_query=True) feeds Mask2Former queries; the HIP path ships the linear-head configs "
                                      "(link_token_to_query=False, rein_dinov2_linear.py:23)")
        if token_length < 2:
            raise ValueError("Reins: token_length must be at least 2 (token 0 is the 'attend to nothing' slot)")
        self.num_layers, self.embed_dims, self.patch_size, self.query_dims = num_layers, embed_dims, patch_size, query_dims
        self.token_length, self.link_token_to_query, self.scale_init = token_length, link_token_to_query, scale_init
        self.use_softmax, self.zero_mlp_delta_f = use_softmax, zero_mlp_delta_f
        self.create_model()

    def create_model(self):
        self.learnable_tokens = nn.Parameter(torch.empty([self.num_layers, self.token_length, self.embed_dims]))
        self.scale = nn.Parameter(torch.tensor(self.scale_init))
        self.mlp_token2feat = nn.Linear(self.embed_dims, self.embed_dims)
        self.mlp_delta_f = nn.Linear(self.embed_dims, self.embed_dims)
        val = math.sqrt(6.0 / float(3 * self.patch_size * self.patch_size + self.embed_dims))
        nn.init.uniform_(self.learnable_tokens.data, -val, val)
        nn.init.kaiming_uniform_(self.mlp_delta_f.weight, a=math.sqrt(5))
        nn.init.kaiming_uniform_(self.mlp_token2feat.weight, a=math.sqrt(5))
        self.transform = nn.Linear(self.embed_dims, self.query_dims)
        self.merge = nn.Linear(self.query_dims * 3, self.query_dims)

    def token_params(self):
        return [self.learnable_tokens]

    def live_params(self):
        """The parameters the adapter step differentiates, in the order DinoEngine hands their gradients back."""
        return self.token_params() + [self.mlp_token2feat.weight, self.mlp_token2feat.bias, self.mlp_delta_f.weight, self.mlp_delta_f.bias,
                                      self.scale]

    def inert_params(self):
        return list(self.transform.parameters()) + list(self.merge.parameters())


@MODELS.register_module()
class LoRAReins(Reins):
    """reins.py:119-148: the tokens of a layer are the product A_l [m, r] @ B_l [r, D]."""

    def __init__(self, lora_dim=16, **kwargs):
        self.lora_dim = lora_dim
        super().__init__(**kwargs)

    def create_model(self):
        super().create_model()
        del self.learnable_tokens
        self.learnable_tokens_a = nn.Parameter(torch.empty([self.num_layers, self.token_length, self.lora_dim]))
        self.learnable_tokens_b = nn.Parameter(torch.empty([self.num_layers, self.lora_dim, self.embed_dims]))
        val = math.sqrt(6.0 / float(3 * self.patch_size * self.patch_size + (self.embed_dims * self.lora_dim) ** 0.5))
        nn.init.uniform_(self.learnable_tokens_a.data, -val, val)
        nn.init.uniform_(self.learnable_tokens_b.data, -val, val)

    def token_params(self):
        return [self.learnable_tokens_a, self.learnable_tokens_b]


@MODELS.register_module()
class ReinsDinoVisionTransformer(DinoVisionTransformer):
    """rein/models/backbones/reins_dinov2.py:7-49: a frozen DINOv2 whose every block is followed by the Rein adapter step on the patch
    tokens (the class token passes through); the taps are taken after the adapter."""

    def __init__(self, reins_config=None, init_cfg=None, **kwargs):
        super().__init__(**kwargs)
        self.reins = MODELS.build(reins_config)
        if self.reins.num_layers != self.n_blocks or self.reins.embed_dims != self.embed_dim:
            raise ValueError("reins_config: num_layers / embed_dims must equal the backbone's depth / embed_dim")
        self._rein_train = False
        # rein_dinov2_linear.py:38-41: the frozen base arrives through init_cfg=dict(type="Pretrained", checkpoint=PATH)
        self.pretrained = None
        ck = init_cfg.get("checkpoint") if isinstance(init_cfg, dict) else None
        if ck is not None:
            if init_cfg.get("type", "Pretrained") != "Pretrained":
                raise NotImplementedError(f"init_cfg type {init_cfg.get('type')!r}: only dict(type='Pretrained', checkpoint=...) is read")
            self.load_pretrained_base(ck)

    def load_pretrained_base(self, checkpoint):
        """The frozen DINOv2 weights (bare keys: cls_token, pos_embed, patch_embed.*, blocks.N.*, ...) from a path or a state dict.  Every
        base parameter must be in it - a file whose keys do not match (a wrong prefix) is an error, not a silently untrained base; the
        `reins.*` keys may be absent (they come from the adapter's own checkpoint or its initialisers)."""
        sd = torch.load(checkpoint, map_location="cpu") if isinstance(checkpoint, (str, os.PathLike)) else checkpoint
        sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
        missing, _ = self.load_state_dict(sd, strict=False)
        missing = [k for k in missing if not k.startswith("reins.")]
        if missing:
            raise RuntimeError(f"pretrained backbone {checkpoint if isinstance(checkpoint, (str, os.PathLike)) else '<state dict>'}: "
                               f"{len(missing)} base parameters not found (first: {missing[:3]}; the file holds e.g. {list(sd)[:3]})")
        self.pretrained = checkpoint if isinstance(checkpoint, (str, os.PathLike)) else "<state dict>"
        self.engine().invalidate()

    def train(self, mode=True):
        """reins_dinov2.py:36-40 + utils.py:9-58: only parameters whose name contains 'reins' are trainable and only the `reins` module is
        in train mode.  `transform` / `merge` never enter the graph (link_token_to_query=False): they stay frozen, like the inert EVA02
        adapters of LoRABackbone.train - torch's AdamW would skip their missing gradients, the flat-buffer optimiser must not decay them."""
        nn.Module.train(self, False)
        self._rein_train = bool(mode)
        if mode:
            for n, p in self.named_parameters():
                p.requires_grad = "reins" in n
            for p in self.reins.inert_params():
                p.requires_grad = False
            self.reins.train(True)
        return self

    def adapter_training(self):
        return self._rein_train

    def full_training(self):
        return False

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        """reins_dinov2.py:42-49: only the keys that contain 'rein' are kept (the frozen base comes from its own checkpoint)."""
        if args:   # torch's deprecated positional form (destination, prefix, keep_vars)
            args = list(args) + [None] * (3 - len(args))
            destination, prefix, keep_vars = args[0], args[1] or "", bool(args[2])
        state = super().state_dict(destination=destination, prefix=prefix, keep_vars=keep_vars)
        for k in [k for k in state.keys() if k.startswith(prefix) and "rein" not in k[len(prefix):]]:
            state.pop(k)
        return state

    def forward(self, x):
        xcat, (hp, wp) = self.forward_tokens([(x, None)], training=self._rein_train)
        b, d = x.shape[0], self.embed_dim
        v = xcat.view(b, hp, wp, len(self.out_indices), d)
        return tuple(v[:, :, :, i].permute(0, 3, 1, 2) for i in range(len(self.out_indices)))


class _Holder(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.model = m


class _PeftModel(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.base_model = _Holder(m)


DINO_LORA_TARGETS = ("qkv", "attn.proj", "fc1", "fc2")   # Lora_config.target_modules the DinoEngine fuses (any non-empty subset)


def check_dino_lora_config(targets, r):
    """What LoRABackbone over a DinoVisionTransformer refuses, by the option's name (no GPU needed to ask)."""
    if not targets:
        raise ValueError(f"Lora_config.target_modules is empty: name at least one of {list(DINO_LORA_TARGETS)}")
    for t in targets:
        if t == "proj":
            raise NotImplementedError("Lora_config.target_modules=['proj'] would also wrap the patch embedding's Conv2d (patch_embed.proj), "
                                      "which is not on the HIP path: write 'attn.proj'")
        if t not in DINO_LORA_TARGETS:
            raise NotImplementedError(f"Lora_config.target_modules: {t!r} is no adapter site of the DinoVisionTransformer HIP engine; "
                                      f"the sites are {list(DINO_LORA_TARGETS)}")
    if not 1 <= int(r) <= R_PAD:
        raise NotImplementedError(f"Lora_config.r={r}: the HIP engine pads the rank to one MFMA K-block, 1 <= r <= {R_PAD}")


@MODELS.register_module()
class LoRABackbone(nn.Module):
    """rein/models/backbones/lora_backbone.py:10-44.  `checkpoint=None` (random init) is accepted - a documented
    deviation: the reference torch.load()s unconditionally."""

    def __init__(self, backbone, checkpoint=None, Lora_config=None, init_cfg=None, **kw):
        super().__init__()
        vit = MODELS.build(backbone)
        cfg = Lora_config or {}
        self.lora_targets = list(cfg.get("target_modules", ["qkv"]))
        if isinstance(vit, DinoVisionTransformer):
            check_dino_lora_config(self.lora_targets, cfg.get("r", 32))
        self.lora_wrapped = []    # dotted names (inside the ViT) of the linear layers that carry an adapter
        # peft: a module is wrapped when its dotted name equals a target or ends with '.' + target
        for name, mod in list(vit.named_modules()):
            if isinstance(mod, _Lin) and any(name == t or name.endswith("." + t) for t in self.lora_targets):
                self.lora_wrapped.append(name)
                parent = vit
                parts = name.split(".")
                for p_ in parts[:-1]:
                    parent = getattr(parent, p_)
                setattr(parent, parts[-1], LoraLinear(mod, cfg.get("r", 32), cfg.get("lora_alpha", 32), cfg.get("lora_dropout", 0.0)))
        if not vit.engine().lora_on():
            raise NotImplementedError(f"target_modules={self.lora_targets}: no adapter site the {type(vit).__name__} HIP engine fuses")
        self.model = _PeftModel(vit)
        self._lora_train = False
        if checkpoint is not None:
            self.load_pretrained_backbone(checkpoint, self.lora_targets)
        self.train(True)

    @property
    def vit(self):
        return self.model.base_model.model

    def load_pretrained_backbone(self, checkpoint, target_modules):
        sd = torch.load(checkpoint, map_location="cpu") if isinstance(checkpoint, str) else checkpoint
        new = {}
        dino = isinstance(self.vit, DinoVisionTransformer)
        wrapped = set(self.lora_wrapped)
        for name, w in sd.items():
            if dino:
                # only the keys of modules that carry an adapter move under `.base_layer` (what lora_backbone.py:30-34 does for these
                # targets by substring): keyed on the wrapped module, no other key - `patch_embed.proj.*` - can ever be renamed with them
                mod, _, leaf = name.rpartition(".")
                if mod in wrapped:
                    name = mod + ".base_layer." + leaf
            else:
                for t in target_modules:  # lora_backbone.py:30-34 rename
                    if t in name:
                        name = name.replace(t, t + ".base_layer")
            new[name] = w
        self.vit.load_state_dict(new, strict=False)
        self.vit.engine().invalidate()

    def train(self, mode=True):
        """lora_backbone.py:37-41 + utils.py:9-58: only parameters whose name contains 'lora' are trainable and the
        base model stays in eval (no drop-path / dropout); modules named lora* (lora_dropout) are in train mode."""
        super().train(False)
        self._lora_train = bool(mode)
        for n, p in self.named_parameters():
            p.requires_grad = ("lora" in n) if mode else p.requires_grad
        if mode:
            # adapters that never enter the graph (EVA02 q/k/v) would only ever see weight decay here;
            # torch's AdamW skips grad-less parameters, so they are simply kept frozen
            for p in getattr(self.vit.engine(), "inert_params", lambda: [])():
                p.requires_grad = False
        return self

    def forward_tokens(self, jobs, seed=None):
        return self.vit.forward_tokens(jobs, training=self._lora_train, seed=seed)

    def forward(self, x):
        xcat, (hp, wp) = self.forward_tokens([(x, None)])
        b, d, nt = x.shape[0], self.vit.embed_dim, len(self.vit.out_indices)
        v = xcat.view(b, hp, wp, nt, d)
        return tuple(v[:, :, :, i].permute(0, 3, 1, 2) for i in range(nt))


# ------------------------------------------------------------------------------------------ packed weights
class Packed:
    """A frozen [N,K] weight in the compute dtype, plus (bf16 mode) its transpose for the dgrad GEMM."""

    def __init__(self, w_f32, cd, k_pad=None):
        n, k = w_f32.shape
        k_pad = k_pad or k
        self.n, self.k = n, k_pad
        self.w = ops.empty_ld(n, k_pad, cd, w_f32.device, zero=True)
        ops.cast(w_f32, self.w[:, :k])
        self.wt = None
        if is_half(cd):
            self.wt = ops.empty_ld(k_pad, n, cd, w_f32.device, zero=True)
            ops.transpose(w_f32, self.wt[:k], pad_rows=n)

    @classmethod
    def alias(cls, w_f32):
        """f32 mode, a TRAINED weight: the operand the GEMMs read IS the optimiser's master (no copy to refresh after a step)."""
        assert w_f32.dtype == torch.float32 and w_f32.dim() == 2 and w_f32.is_contiguous()
        self = cls.__new__(cls)
        self.n, self.k = w_f32.shape
        self.w, self.wt = w_f32, None
        return self

    def fwd(self, a, out, **epi):
        return ops.gemm(a, self.w, out, **epi)

    def dgrad(self, dy, out, **epi):
        if self.wt is not None:
            return ops.gemm(dy, self.wt, out, **epi)
        return ops.gemm(dy, self.w, out, trans_b=True, **epi)

    def dgrad_cols(self, dy, out, c0, c1, **epi):
        """dgrad restricted to the input columns [c0, c1) (a K-extended weight [W | B]: the base part and the LoRA tail apart)."""
        if self.wt is not None:
            return ops.gemm(dy, self.wt[c0:c1], out, **epi)
        return ops.gemm(dy, self.w[:, c0:c1], out, trans_b=True, **epi)


SITE_KEYS = ("qkv", "proj", "fc1", "fc2")   # DinoEngine's adapter sites, in the order of their factors within a block


def _site_mod(blk, key):
    return getattr(blk.attn if key in ("qkv", "proj") else blk.mlp, key)


def _site_ops(key):
    """names of a site's padded A [R_PAD, in] and A^T [in, R_PAD] operands in the packed layer dict"""
    return ("a", "at") if key == "qkv" else ("a_" + key, "at_" + key)


def lora_fused():
    """VFMSEG_LORA_FUSED=1: the sites whose input no LayerNorm kernel produces (attn.proj, fc2) take vfm_lora_down in the 16-bit modes;
    0 (default): the composed dropout_mask + mul_mask + gemm form (always in f32 / bf16x3 storage), which measures faster - 41 against
    82 us at K = 4096, 16.6 against 17.7 ms per all-sites train step - as with VFMSEG_REIN_FUSED."""
    return os.environ.get("VFMSEG_LORA_FUSED", "0") == "1"


def wgrad(dy, x, grad_out, alpha=1.0, n_rows=None, accumulate=True):
    """grad_out[N,K] (+)= alpha * dy[:, :N]^T @ x   (reduction over the M tokens).
    bf16: explicit transposes feed the NT MFMA GEMM (K = tokens, zero-padded to 64); f32: strided operands."""
    M = dy.shape[0]
    res = grad_out if accumulate else None
    if is_half(dy.dtype):
        mp = (M + 63) // 64 * 64
        dyt = torch.empty(dy.shape[1], mp, dtype=dy.dtype, device=dy.device)
        xt = torch.empty(x.shape[1], mp, dtype=x.dtype, device=x.device)
        ops.transpose(dy, dyt, pad_rows=mp)
        ops.transpose(x, xt, pad_rows=mp)
        ops.gemm(dyt, xt, grad_out, alpha=alpha, residual=res)
    else:
        ops.gemm(dy, x, grad_out, alpha=alpha, residual=res, trans_a=True, trans_b=True)
    return grad_out


# ------------------------------------------------------------------------------------------ launch plan of the train step
class _DinoTrainPlan:
    """The backbone's train-step launch sequence (LoRA on, 16-bit mode, fused LN + dropout) as launch plans (ops.Plan -> vfm_run_plan):
    9 launches per block forward, 9-11 backward, over PERSISTENT layer-batched activation buffers, replayed by one C call per pass
    instead of ~430 Python-issued launches (12.2 -> ~6 ms of host enqueue per step).  Same kernels, same arguments,
    same order as DinoEngine.forward / .backward issue one by one: results are bit-identical (tests/test_backbone_gpu.py).
    Buffers (3.9 GB at depth 24, bs 2: 1.4 % of the 288 GB): X[l] the fp32 residual stream entering block l, A1 = [LN1 x | T] the
    K-extended QKV operand, XD the dropped copy, MASK the dropout multiplier, QKV, AO, LSE, XMID, A2, HPRE = gelu'(fc1 pre-activation),
    and for backward DQKV / DA1 of every layer (the batched LoRA weight gradients read them) + DX, T, DH, DN, DAO."""

    def __init__(self, eng, P, nimg, Np):
        v = eng.vit
        cd, dev = P["cd"], P["dev"]
        D, H = v.embed_dim, v.num_heads
        nL = len(v.blocks)
        M, Mp = nimg * Np + nimg, nimg * Np
        Lp0 = P["layers"][0]
        kq, hid = Lp0["qkv"].k, Lp0["fc1"].n
        q0 = v.blocks[0].attn.qkv
        self.eng, self.P, self.nimg, self.Np, self.M, self.Mp, self.nL, self.D, self.H = eng, P, nimg, Np, M, Mp, nL, D, H
        self.busy = False
        e = lambda *sh, dt=cd: torch.empty(*sh, dtype=dt, device=dev)   # noqa: E731
        f32 = torch.float32
        self.X = e(nL + 1, M, D, dt=f32)
        self.A1, self.XD, self.MASK = e(nL, M, kq), e(nL, M, D), e(nL, M, D)
        self.ST1, self.ST2 = e(nL, M, 2, dt=f32), e(nL, M, 2, dt=f32)
        self.QKV, self.AO = e(nL, M, 3 * D), e(nL, M, D)
        self.LSE = e(nL, nimg, H, Np + 1, dt=f32)
        self.XMID, self.A2 = e(nL, M, D, dt=f32), e(nL, M, D)
        hld = hid + ops.ld_pad(hid, cd)
        self.HPRE = e(nL, M, hld)[:, :, :hid]
        self.G = e(M, hld)[:, :hid]
        self.hid, self.kq = hid, kq
        hd = D // H
        scale = hd ** -0.5
        # ---- forward
        f = self.fwd = ops.Plan("backbone")
        self.tap_ops = []     # (plan entry, column offset into xcat): their destination is this step's xcat
        self.nt = len(v.out_indices)
        xcat0 = e(Mp, self.nt * D)   # placeholder destination (patched every step)
        for li, (blk, Lp) in enumerate(zip(v.blocks, P["layers"])):
            q = blk.attn.qkv
            x, a1 = self.X[li], self.A1[li]
            f.layernorm_dropout_fwd(x, Lp["n1w"], Lp["n1b"], 1e-6, a1[:, :D], self.ST1[li], self.XD[li], self.MASK[li], q.p, li * M * D)
            f.gemm(self.XD[li], Lp["a"], a1[:, D:D + R_PAD], alpha=q.scaling)
            f.gemm(a1, Lp["qkv"].w, self.QKV[li], bias=Lp["qkv_b"])
            qkv = self.QKV[li]
            f.attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], self.AO[li], self.LSE[li], nimg, H, hd, Np, 1, Np, 1, scale)
            f.gemm(self.AO[li], Lp["proj"].w, self.XMID[li], bias=Lp["proj_b"], colscale=Lp["g1"], residual=x)
            f.layernorm_fwd(self.XMID[li], Lp["n2w"], Lp["n2b"], 1e-6, self.A2[li], self.ST2[li])
            f.gemm(self.A2[li], Lp["fc1"].w, self.G, bias=Lp["fc1_b"], ep_mode=ops.EP_GELU_DGELU, c2=self.HPRE[li])
            f.gemm(self.G, Lp["fc2"].w, self.X[li + 1], bias=Lp["fc2_b"], colscale=Lp["g2"], residual=self.XMID[li])
            for i, oi in enumerate(v.out_indices):
                if oi == li:
                    self.tap_ops.append((f.cast(self.X[li + 1][:Mp], xcat0[:, i * D:(i + 1) * D]), i * D))
        self.bwd = None

    def eligible_backward(self):
        from .functional import direct_grad_target
        v = self.eng.vit
        return (os.environ.get("VFMSEG_LORA_WGRAD_BATCHED", "1") != "0" and
                all(direct_grad_target(b.attn.qkv.lora_A["default"].weight) is not None and
                    direct_grad_target(b.attn.qkv.lora_B["default"].weight) is not None for b in v.blocks))

    def run_forward(self, xcat, seed, rng0):
        esz = xcat.element_size()
        for idx, col in self.tap_ops:
            self.fwd.entry(idx).u.cast.dst = xcat.data_ptr() + col * esz
        self.fwd.run(seed, rng0)

    def _build_backward(self, dxcat):
        """Two plans: blocks L-1 .. L/2 and L/2-1 .. 0 (the batched LoRA weight gradients of a half, and the DP bucket of the first half,
        go out between them)."""
        v, P = self.eng.vit, self.P
        cd, dev = P["cd"], P["dev"]
        D, H, nL, M, Mp, nimg, Np = self.D, self.H, self.nL, self.M, self.Mp, self.nimg, self.Np
        hd = D // H
        scale = hd ** -0.5
        e = lambda *sh, dt=cd: torch.empty(*sh, dtype=dt, device=dev)   # noqa: E731
        self.DX = e(M, D, dt=torch.float32)
        self.T, self.DN, self.DAO = e(M, D), e(M, D), e(M, D)
        self.DH = e(M, self.hid + ops.ld_pad(self.hid, cd))[:, :self.hid]
        self.DQKV, self.DA1 = e(nL, M, 3 * D), e(nL, M, self.kq)
        half = nL // 2
        skip_l0 = os.environ.get("VFMSEG_PLAN_SKIP_L0", "1") != "0"
        self.half = half
        self.dx_sig = (tuple(dxcat.shape), tuple(dxcat.stride()), dxcat.dtype)
        plans, self.tap_src = [], []      # tap_src: (plan number, entry, column offset into dxcat)

        def add_tap(pl, pn, li):
            for i, oi in enumerate(v.out_indices):
                if oi == li:
                    src = dxcat[:, i * D:(i + 1) * D]
                    self.tap_src.append((pn, pl.strided_copy(src, self.DX, (Mp, D), (src.stride(0), 1), (D, 1), accumulate=True), i * D))

        for pn, (hi, lo) in enumerate(((nL, half), (half, 0)) if half > 0 else ((nL, 0),)):
            pl = ops.Plan("backbone")
            for li in range(hi - 1, lo - 1, -1):
                blk, Lp = v.blocks[li], P["layers"][li]
                q = blk.attn.qkv
                if li == nL - 1:
                    add_tap(pl, pn, li)
                    pl.cast(self.DX, self.T, Lp["g2"])
                pl.gemm(self.T, Lp["fc2"].wt, self.DH, ep_mode=ops.EP_MUL, aux=self.HPRE[li])
                pl.gemm(self.DH, Lp["fc1"].wt, self.DN)
                pl.layernorm_bwd_scaled(self.DN, self.XMID[li], Lp["n2w"], self.ST2[li], self.DX, self.T, Lp["g1"], accumulate_dx=True)
                pl.gemm(self.T, Lp["proj"].wt, self.DAO)
                qkv, dqkv, da1 = self.QKV[li], self.DQKV[li], self.DA1[li]
                pl.attn_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], self.AO[li], self.LSE[li], self.DAO, dqkv[:, :D], dqkv[:, D:2 * D],
                            dqkv[:, 2 * D:], nimg, H, hd, Np, 1, Np, 1, scale)
                if li == 0 and skip_l0:
                    # block 0: nothing upstream of LN1 is trainable (patch embedding, position embedding and [cls] token are frozen,
                    # lora_backbone.py:36-44), so of d[LN1 x | T] only dT - the LoRA factors' gradient operand - is needed: 64 of the 1088
                    # columns of the qkv input gradient, no LoRA dgrad GEMM, no LN1 backward
                    pl.gemm(dqkv, Lp["qkv"].wt[D:D + R_PAD], da1[:, D:D + R_PAD])
                    continue
                pl.gemm(dqkv, Lp["qkv"].wt, da1)
                pl.gemm(da1[:, D:D + R_PAD], Lp["at"], da1[:, :D], alpha=q.scaling, residual=da1[:, :D], ep_mode=ops.EP_MUL, aux=self.MASK[li])
                if li > 0:
                    add_tap(pl, pn, li - 1)
                    pl.layernorm_bwd_scaled(da1[:, :D], self.X[li], Lp["n1w"], self.ST1[li], self.DX, self.T, P["layers"][li - 1]["g2"],
                                            accumulate_dx=True)
                else:   # (the one-by-one path's LN1 backward of block 0; its dx is not used by anything)
                    pl.layernorm_bwd_scaled(da1[:, :D], self.X[li], Lp["n1w"], self.ST1[li], self.DX, self.T, Lp["g2"], accumulate_dx=True)
            plans.append((pl, lo, hi))
        self.bwd = plans

    def run_backward(self, ctx, dxcat):
        sig = (tuple(dxcat.shape), tuple(dxcat.stride()), dxcat.dtype)
        if self.bwd is None or self.dx_sig != sig:
            self._build_backward(dxcat)
        esz = dxcat.element_size()
        for pn, idx, col in self.tap_src:
            self.bwd[pn][0].entry(idx).u.copy.src = dxcat.data_ptr() + col * esz
        self.DX.zero_()
        for pl, lo, hi in self.bwd:
            pl.run()
            self.eng._lora_wgrads_batched(self.P, ctx, self.DA1, self.DQKV, lo, hi, self.M, self.D)
            if BACKWARD_EVENTS["block_done"] is not None:
                for lj in range(hi - 1, lo - 1, -1):
                    BACKWARD_EVENTS["block_done"](lj)


# ------------------------------------------------------------------------------------------ engine
class DinoEngine:
    def __init__(self, vit):
        self.vit = vit
        self._packed = None
        self._pos_cache = {}

    def invalidate(self):
        self._packed = None
        self._pos_cache = {}

    def sites(self):
        """The adapted linear layers of a block (LoRABackbone wraps the same ones in every block), in SITE_KEYS order."""
        b0 = self.vit.blocks[0]
        return tuple(k for k in SITE_KEYS if isinstance(_site_mod(b0, k), LoraLinear))

    def lora_on(self):
        return bool(self.sites())

    def rein_on(self):
        return getattr(self.vit, "reins", None) is not None

    def bare(self):
        return not self.lora_on() and not self.rein_on()

    def full_on(self):
        return self.bare() and getattr(self.vit, "full_training", lambda: False)()

    def full_params(self):
        """The base parameters that enter the graph, in the fixed order _backward_full hands their gradients back: the embeddings, then per
        block norm1, qkv, proj, ls1, norm2, fc1, fc2, ls2 (absent biases are left out)."""
        v = self.vit
        out = [v.patch_embed.proj.weight, v.patch_embed.proj.bias, v.cls_token, v.pos_embed]
        for blk in v.blocks:
            out += [blk.norm1.weight, blk.norm1.bias, blk.attn.qkv.weight, blk.attn.qkv.bias, blk.attn.proj.weight, blk.attn.proj.bias,
                    blk.ls1.gamma, blk.norm2.weight, blk.norm2.bias, blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight,
                    blk.mlp.fc2.bias, blk.ls2.gamma]
        return [p for p in out if p is not None]

    def check_full_training(self, hp, wp):
        """What full fine-tuning refuses, by the option's name (no GPU needed to ask)."""
        from .precision import split3 as _x3_mode
        v = self.vit
        if v.drop_path_rate > 0:
            raise NotImplementedError(f"drop_path_rate={v.drop_path_rate}: stochastic depth is not on the HIP training path; full fine-tuning "
                                      "of DinoVisionTransformer needs drop_path_rate=0")
        if _x3_mode():
            raise NotImplementedError("precision mode 'bf16x3' is a prediction mode: full fine-tuning of DinoVisionTransformer runs in "
                                      "f32, bf16 or fp16")
        s = int(math.sqrt(v.pos_embed.shape[1] - 1))
        if (hp, wp) != (s, s):
            raise NotImplementedError(f"img_size={v.img_size}: the training token grid {hp}x{wp} differs from the pos_embed grid {s}x{s}; "
                                      "the pos_embed gradient would have to pass back through the bicubic interpolation - train crops of "
                                      "img_size (the reference trains 512x512 crops at img_size=512)")

    def trainable(self):
        out = []
        if self.full_on():
            return self.full_params()
        sites = self.sites()
        for blk in (self.vit.blocks if sites else ()):   # block order; within a block qkv, proj, fc1, fc2 (backward() hands back this order)
            for k in sites:
                m = _site_mod(blk, k)
                out += [m.lora_A["default"].weight, m.lora_B["default"].weight]
        if self.rein_on():   # (after the per-block LoRA factors: backward() returns its gradients in this order)
            out += self.vit.reins.live_params()
        return out

    # ---- frozen weights, packed once per (dtype, device)
    def packed(self):
        cd = compute_dtype()
        dev = self.vit.pos_embed.device
        v = self.vit
        # a TRAINED base (bare backbone whose weights require gradients): the fp32 vectors alias the master, the packed 2-D images are
        # rewritten after every optimiser step (one launch: ops.PackTable), keyed on PARAM_EPOCH like the decoder heads' pack cache
        tb = self.bare() and v.patch_embed.proj.weight.requires_grad
        P = self._packed
        if P is not None and P["cd"] == cd and P["dev"] == dev and P.get("trained", False) == tb:
            if not tb:
                return P
            if P["ptrs"] == [p.data_ptr() for p in self.full_params()]:
                from .optim import PARAM_EPOCH
                key = (PARAM_EPOCH[0], sum(p._version for p in P["params"]))
                if P["epoch"] != key:
                    if P["pack_table"] is not None:
                        P["pack_table"].run()
                    P["epoch"] = key
                    self._pos_cache = {}    # (position embeddings interpolated to other grids: the embedding moved)
                return P
        D = v.embed_dim
        P = dict(cd=cd, dev=dev, layers=[], trained=tb)
        if tb:
            return self._pack_trained(P)
        with torch.no_grad():
            pw = v.patch_embed.proj.weight.detach().reshape(D, -1)
            P["pe"] = Packed(pw, cd)
            P["pe_b"] = v.patch_embed.proj.bias.detach().float().contiguous()
            P["cls"] = v.cls_token.detach().reshape(D).float().contiguous()
            for blk in v.blocks:
                Lp = {}
                for key in SITE_KEYS:   # an adapted site's weight is packed as [W | B]: K extended by the padded rank
                    m = _site_mod(blk, key)
                    base = m.base_layer if isinstance(m, LoraLinear) else m
                    kin = base.in_features
                    Lp[key] = Packed(base.weight.detach(), cd, k_pad=kin + (R_PAD if isinstance(m, LoraLinear) else 0))
                    Lp[key + "_b"] = base.bias.detach().float().contiguous() if base.bias is not None else None
                    if isinstance(m, LoraLinear):
                        na, nat = _site_ops(key)
                        Lp[na] = torch.zeros(R_PAD, kin, dtype=cd, device=dev)       # A padded to 64 rows   [r, in]
                        Lp[nat] = torch.zeros(kin, R_PAD, dtype=cd, device=dev)      # A^T                   [in, r]
                Lp.update(
                    g1=blk.ls1.gamma.detach().float().contiguous(), g2=blk.ls2.gamma.detach().float().contiguous(),
                    n1w=blk.norm1.weight.detach().float().contiguous(), n1b=blk.norm1.bias.detach().float().contiguous(),
                    n2w=blk.norm2.weight.detach().float().contiguous(), n2b=blk.norm2.bias.detach().float().contiguous(),
                )
                P["layers"].append(Lp)
        self._packed = P
        return P

    def _pack_trained(self, P):
        """packed() of a trained base.  Every fp32 vector (biases, LayerNorm / LayerScale weights, cls, pos) IS the parameter's storage - the
        optimiser's flat master once FusedAdamW has re-pointed it - and so is, in the f32 mode, every 2-D GEMM operand (Packed.alias).  In
        the 16-bit modes the 2-D images are Packed(...) as for a frozen base, and P["pack_table"] rewrites all of them from the master in
        one launch: the same conversions, hence the same bits, as building them afresh."""
        from .optim import PARAM_EPOCH
        v = self.vit
        cd, D = P["cd"], v.embed_dim
        params = self.full_params()
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("full fine-tuning needs contiguous fp32 backbone parameters (the packed operands alias or follow them)")
        sites = []

        def pack(w):
            w = w.detach()
            w2 = w.reshape(w.shape[0], -1)
            if cd == torch.float32:
                return Packed.alias(w2)
            pk = Packed(w2, cd)
            sites.append((w2, pk.w, pk.wt))
            return pk

        vec = lambda p: None if p is None else p.detach().reshape(-1)   # noqa: E731
        with torch.no_grad():
            P["pe"] = pack(v.patch_embed.proj.weight)
            P["pe_b"] = vec(v.patch_embed.proj.bias)
            P["cls"] = vec(v.cls_token)
            for blk in v.blocks:
                P["layers"].append(dict(
                    qkv=pack(blk.attn.qkv.weight), qkv_b=vec(blk.attn.qkv.bias), proj=pack(blk.attn.proj.weight), proj_b=vec(blk.attn.proj.bias),
                    fc1=pack(blk.mlp.fc1.weight), fc1_b=vec(blk.mlp.fc1.bias), fc2=pack(blk.mlp.fc2.weight), fc2_b=vec(blk.mlp.fc2.bias),
                    g1=vec(blk.ls1.gamma), g2=vec(blk.ls2.gamma), n1w=vec(blk.norm1.weight), n1b=vec(blk.norm1.bias),
                    n2w=vec(blk.norm2.weight), n2b=vec(blk.norm2.bias)))
        P["ptrs"] = [p.data_ptr() for p in params]
        P["params"] = params
        P["pack_table"] = ops.PackTable(sites) if sites else None
        P["epoch"] = (PARAM_EPOCH[0], sum(p._version for p in params))
        self._packed = P
        return P

    def refresh_lora(self, P):
        """LoRA factors change every optimiser step: re-pack them into the concatenated operands of every adapted site (one launch)."""
        sites = []
        keys = self.sites()
        for blk, Lp in zip(self.vit.blocks, P["layers"]):
            for key in keys:
                q = _site_mod(blk, key)
                na, nat = _site_ops(key)
                A, Bm = q.lora_A["default"].weight.detach(), q.lora_B["default"].weight.detach()
                sites.append((A, Bm, Lp[na], Lp[nat], Lp[key].w, Lp[key].wt, q.r, A.shape[1], Bm.shape[0], A.shape[1]))
        _refresh_sites(P, sites)

    def merged_weights(self, P):
        """Inference only (no LoRA dropout): per adapted site and layer the compute-dtype copy of W + s * B A, so that the projection is
        ONE GEMM of the base shape (no T = x A^T product, no K extension).  Rebuilt when a LoRA factor changed (torch version counters,
        data pointers, and the optimiser's epoch for the fused AdamW kernel that updates parameters behind torch's back).
        Returns {site: [per-layer weight]}."""
        from .optim import PARAM_EPOCH
        keys = self.sites()
        key = [PARAM_EPOCH[0], keys]
        for blk in self.vit.blocks:
            for k in keys:
                q = _site_mod(blk, k)
                A, Bm = q.lora_A["default"].weight, q.lora_B["default"].weight
                key += [A._version, Bm._version, A.data_ptr(), Bm.data_ptr()]
        key = tuple(key)
        if P.get("merged_key") == key:
            return P["merged"]
        cd, dev = P["cd"], P["dev"]
        merged = {k: [] for k in keys}
        with torch.no_grad():
            for blk in self.vit.blocks:
                for k in keys:
                    q = _site_mod(blk, k)
                    A, Bm = q.lora_A["default"].weight.detach().float(), q.lora_B["default"].weight.detach().float()
                    w = q.base_layer.weight.detach().float()
                    weff = torch.empty_like(w)
                    ops.gemm(Bm.contiguous(), A.contiguous(), weff, alpha=q.scaling, residual=w, trans_b=True)   # W + s * B A   (fp32 MFMA)
                    wp = ops.empty_ld(w.shape[0], w.shape[1], cd, dev)
                    ops.cast(weff, wp)
                    merged[k].append(wp)
        P["merged"], P["merged_key"] = merged, key
        return merged

    def pos_tokens(self, hp, wp):
        v = self.vit
        n = v.pos_embed.shape[1] - 1
        s = int(math.sqrt(n))
        if hp == s and wp == s:
            return v.pos_embed.detach().reshape(n + 1, -1).float().contiguous()
        key = (hp, wp)
        if key not in self._pos_cache:
            # dino_v2.py:184-215: bicubic with scale_factor = (h0 + 0.1) / sqrt(N); F.interpolate maps coordinates with
            # 1 / scale_factor.  The pos-embed is frozen, so the result is cached per token grid.
            D = v.embed_dim
            pe = v.pos_embed.detach().reshape(n + 1, D).float().contiguous()
            out = torch.empty(1 + hp * wp, D, dtype=torch.float32, device=pe.device)
            ops.cast(pe[:1], out[:1])
            sy, sx = s / (hp + 0.1), s / (wp + 0.1)
            assert int(s * ((hp + 0.1) / s)) == hp and int(s * ((wp + 0.1) / s)) == wp
            ops.resize_bicubic(pe[1:], s, s, D, out[1:], hp, wp, sy, sx)
            self._pos_cache[key] = out
        return self._pos_cache[key]

    # ---- forward
    def forward(self, jobs, training, seed, need_grad=False):
        v, P = self.vit, self.packed()
        cd = P["cd"]
        dev = P["dev"]
        D, H, ps = v.embed_dim, v.num_heads, v.patch_size
        sites = self.sites()
        lora = "qkv" in sites      # (the QKV site: the LN1-fed branch below; the other sites are `ext`)
        rein = self._rein_pack(P) if self.rein_on() else None
        merged = None
        from .precision import split3 as _x3_mode
        x3 = _x3_mode() and not is_half(cd)
        if (sites and not training and not torch.is_grad_enabled() and (is_half(cd) or x3)
                and os.environ.get("VFMSEG_MERGE_LORA_EVAL", "1") != "0"):
            merged = self.merged_weights(P)
        elif sites:
            self.refresh_lora(P)
        sizes = []
        for img, box in jobs:
            y0, y1, x0, x1 = box if box is not None else (0, img.shape[2], 0, img.shape[3])
            sizes.append(((y1 - y0) // ps, (x1 - x0) // ps))
        hp, wp = sizes[0]
        assert all(s == (hp, wp) for s in sizes), "all jobs of one backbone call must share the token grid"
        Np = hp * wp
        full = bool(training and need_grad and self.full_on())   # the base itself is trained: keep what its weight gradients read
        if full:
            self.check_full_training(hp, wp)
        nimg = sum(j[0].shape[0] for j in jobs)
        Mp, M = nimg * Np, nimg * Np + nimg
        kpe = 3 * ps * ps
        A0 = torch.empty(Mp, kpe, dtype=cd, device=dev)
        r0 = 0
        for img, box in jobs:
            b = img.shape[0]
            ops.patchify(img, A0[r0 * Np:(r0 + b) * Np], box=box, patch=ps)
            r0 += b
        ptok = torch.empty(Mp, D, dtype=torch.float32, device=dev)
        P["pe"].fwd(A0, ptok, bias=P["pe_b"])
        plan = self._train_plan(P, nimg, Np, training, merged) if need_grad else None
        x = plan.X[0] if plan is not None else torch.empty(M, D, dtype=torch.float32, device=dev)
        ops.assemble_tokens(ptok, P["cls"], self.pos_tokens(hp, wp), x, nimg, Np, D)
        del ptok
        if not full:
            del A0    # (full fine-tuning: the patch rows are the patch embedding's weight-gradient operand)
        nt = len(v.out_indices)
        from .precision import eval_heads_fp32
        tap_dt = torch.float32 if (not training and not need_grad and eval_heads_fp32()) else cd
        xcat = torch.empty(Mp, nt * D, dtype=tap_dt, device=dev)
        saved = []
        hid = P["layers"][0]["fc1"].n
        # dropout counters: one region of nL * M * width per site, laid end to end in SITE_KEYS order (disjoint streams); a call reserves up
        # to the end of its last adapted site - a qkv-only model nL * M * D, its seeds, offsets and masks are what they always were
        rng_site, end, rng_n = {}, 0, 0
        for k in SITE_KEYS:
            rng_site[k] = end
            end += len(v.blocks) * M * (hid if k == "fc2" else D)
            if k in sites:
                rng_n = end
        if sites and training:
            from .functional import draw_seed
            seed, rng0 = draw_seed(seed, rng_n)
        else:
            seed, rng0 = 0, 0
        if plan is not None:
            plan.run_forward(xcat, seed, rng0)
            plan.busy = True
            ctx = dict(saved=None, plan=plan, nimg=nimg, Np=Np, M=M, Mp=Mp, P=P, training=training, A1all=plan.A1, XDall=plan.XD)
            return xcat, (hp, wp), ctx
        # training: the K-extended QKV operands [LN(x) | T] and the dropped LN copies of ALL layers live in two layer-batched
        # buffers, so that the LoRA weight gradients of many layers can run as ONE batched GEMM each (see backward)
        nL = len(v.blocks)
        batched = lora and training and is_half(cd) and merged is None
        A1all = torch.empty(nL, M, P["layers"][0]["qkv"].k, dtype=cd, device=dev) if batched else None
        XDall = None
        hd = D // H
        scale = hd ** -0.5
        for li, (blk, Lp) in enumerate(zip(v.blocks, P["layers"])):
            S = {"x_in": x}
            kq = D if merged is not None else Lp["qkv"].k
            # [LN(x) | T]: the T GEMM writes all R_PAD columns (A is zero-padded)
            a1 = A1all[li] if batched else torch.empty(M, kq, dtype=cd, device=dev)
            st1 = torch.empty(M, 2, dtype=torch.float32, device=dev)
            q = blk.attn.qkv if lora else None
            fused_drop = lora and training and q.p > 0 and is_half(cd) and D % 256 == 0
            if fused_drop:  # LN + dropout multiplier + dropped copy in one pass
                mask = torch.empty(M, D, dtype=cd, device=dev)
                if batched and XDall is None:
                    XDall = torch.empty(nL, M, D, dtype=cd, device=dev)
                xd = XDall[li] if batched else torch.empty(M, D, dtype=cd, device=dev)
                ops.layernorm_dropout_fwd(x, Lp["n1w"], Lp["n1b"], 1e-6, a1[:, :D], st1, xd, mask, q.p, seed, offset=rng0 + li * M * D)
            else:
                # bf16x3 predictions: outputs whose one consumer is a GEMM's A operand leave their producer as split-bf16 images
                so = "only" if (x3 and not training and not need_grad and kq == D) else None
                ops.layernorm_fwd(x, Lp["n1w"], Lp["n1b"], 1e-6, a1 if kq == D else a1[:, :D], st1, split_out=so)
            if lora and merged is None:
                if not fused_drop:
                    xd, mask = a1[:, :D], None
                    if training and q.p > 0:
                        mask = torch.empty(M, D, dtype=cd, device=dev)
                        ops.dropout_mask(mask, q.p, seed, offset=rng0 + li * M * D)
                        xd = torch.empty(M, D, dtype=cd, device=dev)
                        ops.mul_mask(a1[:, :D], mask, xd)
                ops.gemm(xd, Lp["a"], a1[:, D:D + R_PAD], alpha=q.scaling)  # T = s * drop(xn) A^T
                S.update(xd=xd if mask is not None else None, mask=mask)
            qkv = torch.empty(M, 3 * D, dtype=cd, device=dev)
            if merged is not None and lora:
                ops.gemm(a1, merged["qkv"][li], qkv, bias=Lp["qkv_b"])
            else:
                Lp["qkv"].fwd(a1, qkv, bias=Lp["qkv_b"])
            # the other adapter sites, unmerged: the operand is [x | T] with x the site's input in the first K columns of a buffer whose
            # leading dimension is K + R_PAD (the producers below write strided views) and the weight is packed as [W | B]
            ext = {k: (k in sites and merged is None) for k in ("proj", "fc1", "fc2")}
            S["lora"] = {}
            ao_op = torch.empty(M, D + (R_PAD if ext["proj"] else 0), dtype=cd, device=dev)
            ao = ao_op[:, :D] if ext["proj"] else ao_op
            lse = torch.empty(nimg, H, Np + 1, dtype=torch.float32, device=dev)
            so = "only" if (x3 and not training and not need_grad) else None
            ops.attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], ao, lse, nimg, H, hd, Np, 1, Np, 1, scale, keep_split=training,
                         o_split=None if ext["proj"] else so)
            if ext["proj"]:
                S["lora"]["proj"] = self._lora_down(blk.attn.proj, Lp["a_proj"], ao_op, D, training, seed, rng0 + rng_site["proj"] + li * M * D)
            xm = torch.empty(M, D, dtype=torch.float32, device=dev)
            # full fine-tuning: the epilogue's second output is the branch output BEFORE the LayerScale column scale (bias included) -
            # what d gamma reads; x_mid / x_out themselves are what every other caller gets
            u1 = torch.empty(M, D, dtype=cd, device=dev) if full else None
            u2 = torch.empty(M, D, dtype=cd, device=dev) if full else None
            if merged is not None and "proj" in sites:
                ops.gemm(ao, merged["proj"][li], xm, bias=Lp["proj_b"], colscale=Lp["g1"], residual=x)
            else:
                Lp["proj"].fwd(ao_op, xm, bias=Lp["proj_b"], colscale=Lp["g1"], residual=x, **({"c2": u1} if full else {}))
            a2_op = torch.empty(M, D + (R_PAD if ext["fc1"] else 0), dtype=cd, device=dev)
            a2 = a2_op[:, :D] if ext["fc1"] else a2_op
            st2 = torch.empty(M, 2, dtype=torch.float32, device=dev)
            if ext["fc1"]:    # fed by LayerNorm 2 as the QKV site is by LayerNorm 1: LN + dropout multiplier + dropped copy in one pass
                q1 = blk.mlp.fc1
                off1 = rng0 + rng_site["fc1"] + li * M * D
                xd1 = mask1 = None
                if training and q1.p > 0:
                    mask1, xd1 = torch.empty(M, D, dtype=cd, device=dev), torch.empty(M, D, dtype=cd, device=dev)
                    if is_half(cd) and D % 256 == 0:
                        ops.layernorm_dropout_fwd(xm, Lp["n2w"], Lp["n2b"], 1e-6, a2, st2, xd1, mask1, q1.p, seed, offset=off1)
                    else:
                        ops.layernorm_fwd(xm, Lp["n2w"], Lp["n2b"], 1e-6, a2, st2)
                        ops.dropout_mask(mask1, q1.p, seed, offset=off1)
                        ops.mul_mask(a2, mask1, xd1)
                else:
                    ops.layernorm_fwd(xm, Lp["n2w"], Lp["n2b"], 1e-6, a2, st2)
                ops.gemm(xd1 if xd1 is not None else a2, Lp["a_fc1"], a2_op[:, D:D + R_PAD], alpha=q1.scaling)
                S["lora"]["fc1"] = (xd1, mask1)
            else:
                ops.layernorm_fwd(xm, Lp["n2w"], Lp["n2b"], 1e-6, a2, st2, split_out=so)
            g_op =torch.empty(M, hid + R_PAD, dtype=cd, device=dev) if ext["fc2"] else None
            g = g_op[:, :hid] if ext["fc2"] else ops.empty_ld(M, hid, cd, dev)
            w1 = merged["fc1"][li] if (merged is not None and "fc1" in sites) else Lp["fc1"].w
            if training and (sites or (rein is not None and need_grad) or full):   # the forward also saves gelu'(pre-activation): what fc2's dgrad multiplies by (mlp.py:34-40)
                hpre = torch.empty(M, hid, dtype=cd, device=dev)
                ops.gemm(a2_op, w1, g, bias=Lp["fc1_b"], ep_mode=ops.EP_GELU_DGELU, c2=hpre)
            else:
                hpre = None
                ops.gemm(a2_op, w1, g, bias=Lp["fc1_b"], ep_mode=ops.EP_GELU, **({"c_split": so} if (so and not ext["fc2"]) else {}))
            if ext["fc2"]:
                S["lora"]["fc2"] = self._lora_down(blk.mlp.fc2, Lp["a_fc2"], g_op, hid, training, seed, rng0 + rng_site["fc2"] + li * M * hid)
            xo = torch.empty(M, D, dtype=torch.float32, device=dev)
            if merged is not None and "fc2" in sites:
                ops.gemm(g, merged["fc2"][li], xo, bias=Lp["fc2_b"], colscale=Lp["g2"], residual=xm)
            else:
                Lp["fc2"].fwd(g_op if ext["fc2"] else g, xo, bias=Lp["fc2_b"], colscale=Lp["g2"], residual=xm, **({"c2": u2} if full else {}))
            S.update(ao_op=ao_op, a2_op=a2_op, g_op=g_op)
            S.update(a1=a1, st1=st1, qkv=qkv, ao=ao, lse=lse, x_mid=xm, a2=a2, st2=st2, hpre=hpre, g=g, u1=u1, u2=u2)
            saved.append(S)
            x = xo
            if rein is not None:   # the adapter step on the patch rows; the taps below read its output (reins_dinov2.py:22-33)
                x = self._rein_forward(rein, li, x, Mp, S if (training and need_grad) else None)
            for i, oi in enumerate(v.out_indices):   # (an index may be listed more than once: every copy is a tap of its own)
                if oi == li:
                    ops.cast(x[:Mp], xcat[:, i * D:(i + 1) * D])
        ctx = dict(saved=saved, nimg=nimg, Np=Np, M=M, Mp=Mp, P=P, training=training, A1all=A1all, XDall=XDall, rein=rein,
                   full=full, A0=A0 if full else None)
        return xcat, (hp, wp), ctx

    @staticmethod
    def _lora_down(q, a_op, buf, K, training, seed, offset):
        """buf [M, K + R_PAD] holds the adapter input x of site q in its first K columns; writes T = s * drop(x) A^T into the K tail (all
        R_PAD columns: A is zero-padded).  Returns (xd, mask) - the dropped copy and the multiplier backward reads - or (None, None)
        without dropout.  dropout_mask + mul_mask + gemm, or with VFMSEG_LORA_FUSED=1 in the 16-bit modes ONE launch (vfm_lora_down),
        which writes the same mask and xd bits."""
        x, T = buf[:, :K], buf[:, K:K + R_PAD]
        drop = bool(training and q.p > 0)
        xd = mask = None
        if drop:
            mask = torch.empty(x.shape[0], K, dtype=x.dtype, device=x.device)
            xd = torch.empty(x.shape[0], K, dtype=x.dtype, device=x.device)
        if lora_fused() and ops.lora_down_ok(x, a_op):
            ops.lora_down(x, a_op, T, q.scaling, q.p if drop else 0.0, seed, offset, mask, xd)
        else:
            if drop:
                ops.dropout_mask(mask, q.p, seed, offset=offset)
                ops.mul_mask(x, mask, xd)
            ops.gemm(xd if drop else x, a_op, T, alpha=q.scaling)
        return xd, mask

    def _train_plan(self, P, nimg, Np, training, merged):
        """The launch plan of this call's shape when the call is the hot one (training with gradients, LoRA on the QKV site alone with
        dropout on every block, 16-bit mode, weight gradients into the optimiser's flat buffer) and no earlier forward still owns the
        plan's buffers.  Other adapter sites run on the one-by-one path."""
        v = self.vit
        if (not training or merged is not None or self.sites() != ("qkv",) or self.rein_on() or not is_half(P["cd"])
                or os.environ.get("VFMSEG_PLAN", "1") == "0" or v.embed_dim % 256 != 0):
            return None
        q0 = v.blocks[0].attn.qkv
        if not all(isinstance(b.attn.qkv, LoraLinear) and b.attn.qkv.p > 0 and b.attn.qkv.p == q0.p and b.attn.qkv.scaling == q0.scaling
                   for b in v.blocks):
            return None
        plans = P.setdefault("plans", {})
        pl = plans.get((nimg, Np))
        if pl is None:
            pl = plans[(nimg, Np)] = _DinoTrainPlan(self, P, nimg, Np)
        if pl.busy or not pl.eligible_backward():
            return None
        return pl

    # ---- backward: d(xcat) -> LoRA grads [dA0, dB0, dA1, dB1, ...]
    def backward(self, ctx, dxcat):
        if ctx.get("plan") is not None:
            plan = ctx["plan"]
            try:
                plan.run_backward(ctx, dxcat)
            finally:
                plan.busy = False
            return [None] * (2 * len(self.vit.blocks))      # (the plan runs qkv-only models)
        if ctx.get("full"):
            return self._backward_full(ctx, dxcat)
        v, P = self.vit, ctx["P"]
        cd, dev = P["cd"], P["dev"]
        D, H = v.embed_dim, v.num_heads
        hd = D // H
        scale = hd ** -0.5
        M, Mp, nimg, Np = ctx["M"], ctx["Mp"], ctx["nimg"], ctx["Np"]
        dx = torch.zeros(M, D, dtype=torch.float32, device=dev)
        sites = self.sites()
        ns = len(sites)
        grads = [None] * (2 * ns * len(v.blocks))    # trainable() order: per block, per adapted site, (A, B)
        gidx = {k: 2 * i for i, k in enumerate(sites)}
        nL = len(v.blocks)
        rein = ctx.get("rein")
        rein_acc = self._rein_backward_begin(rein) if rein is not None else None
        # LoRA weight gradients, layer-batched: dB_l^T = T_l^T dqkv_l and dA_l = s dT_l^T drop(LN x)_l are 2 x 24 skinny GEMMs
        # (64 output rows, reduction over the 4100 tokens) that each needed split-K slabs + a combine launch (35 us per layer for
        # 0.3 % of the step's FLOPs).  Keeping dqkv / d[LN x | T] of the layers (0.8 GB of 288) turns them into TWO batched GEMMs
        # per half of the backbone - no split-K, no slabs - plus one batched scatter into the flat gradient buffer.  Two halves so
        # that the first LoRA gradient bucket can still leave (DP) while the second half of the backward runs.
        from .functional import direct_grad_target
        wg_batched = (ctx.get("A1all") is not None and "qkv" in sites and os.environ.get("VFMSEG_LORA_WGRAD_BATCHED", "1") != "0" and
                      all(direct_grad_target(b.attn.qkv.lora_A["default"].weight) is not None and
                          direct_grad_target(b.attn.qkv.lora_B["default"].weight) is not None for b in v.blocks) and
                      (ctx.get("XDall") is not None or all(S_["mask"] is None for S_ in ctx["saved"])))
        if wg_batched:
            kq_all = ctx["A1all"].shape[2]
            DA1all = torch.empty(nL, M, kq_all, dtype=cd, device=dev)
            DQKVall = torch.empty(nL, M, 3 * D, dtype=cd, device=dev)
        half = nL // 2
        fuse_t = is_half(cd) and D % 256 == 0  # LN backward emits the next dgrad operand bf16(dx * gamma) itself
        # with an adapter between block li-1 and li the tap gradient belongs to the adapter's OUTPUT and the adapter's backward rewrites dx
        # before t = bf16(dx * g2) may be formed: the LN1 backward then must not emit t for the block below
        fuse_t1 = fuse_t and rein is None
        def add_tap(li):
            for i, oi in enumerate(v.out_indices):
                if oi == li:
                    src = dxcat[:, i * D:(i + 1) * D]
                    ops.strided_copy(src, dx, (Mp, D), (src.stride(0), 1), (D, 1), accumulate=True)
        t = None
        for li in range(len(v.blocks) - 1, -1, -1):
            blk, Lp, S = v.blocks[li], P["layers"][li], ctx["saved"][li]
            q = blk.attn.qkv
            # ---- MLP branch: x_out = x_mid + g2 * fc2(gelu(fc1(LN2(x_mid))))
            if t is None:  # (the previous iteration's LN1 backward already produced t = bf16(dx * g2) otherwise)
                add_tap(li)
                if rein is not None:
                    self._rein_backward(rein, rein_acc, li, dx, Mp, S)
                t = torch.empty(M, D, dtype=cd, device=dev)
                ops.cast(dx, t, Lp["g2"])
            hid = Lp["fc1"].n
            dh = ops.empty_ld(M, hid, cd, dev)
            SL = S.get("lora") or {}
            g0 = 2 * ns * li
            if "fc2" in SL:
                # d g = t [W | B] has the base part dg0 = t W and the tail dT = t B; d h = gelu'(pre) * (dg0 + mask * (s dT A)): the first
                # term is the dgrad epilogue as ever, the second the site's EP_MUL GEMM with gelu'(pre) * mask as its multiplier
                xd2, mask2 = SL["fc2"]
                Lp["fc2"].dgrad_cols(t, dh, 0, hid, ep_mode=ops.EP_MUL, aux=S["hpre"])
                dT2 = torch.empty(M, R_PAD, dtype=cd, device=dev)
                Lp["fc2"].dgrad_cols(t, dT2, hid, hid + R_PAD)
                mul2 = S["hpre"]
                if mask2 is not None:
                    mul2 = torch.empty_like(S["hpre"])
                    ops.mul_mask(S["hpre"], mask2, mul2)
                self._site_backward(blk.mlp.fc2, Lp["at_fc2"], S["g_op"][:, hid:hid + R_PAD], t, dT2, dh,
                                    xd2 if xd2 is not None else S["g"], mul2, grads, g0 + gidx["fc2"])
            else:
                Lp["fc2"].dgrad(t, dh, ep_mode=ops.EP_MUL, aux=S["hpre"])
            dn_op = torch.empty(M, Lp["fc1"].k, dtype=cd, device=dev)
            Lp["fc1"].dgrad(dh, dn_op)
            dn = dn_op[:, :D] if "fc1" in SL else dn_op
            if "fc1" in SL:
                xd1, mask1 = SL["fc1"]
                self._site_backward(blk.mlp.fc1, Lp["at_fc1"], S["a2_op"][:, D:D + R_PAD], dh, dn_op[:, D:D + R_PAD], dn,
                                    xd1 if xd1 is not None else S["a2"], mask1, grads, g0 + gidx["fc1"])
            if fuse_t:
                ops.layernorm_bwd_scaled(dn, S["x_mid"], Lp["n2w"], S["st2"], dx, t, Lp["g1"], accumulate_dx=True)
            else:
                ops.layernorm_bwd(dn, S["x_mid"], Lp["n2w"], S["st2"], dx, accumulate_dx=True)
                ops.cast(dx, t, Lp["g1"])
            del dh
            # ---- attention branch: x_mid = x_in + g1 * proj(attn(qkv(LN1(x_in))))
            dao_op = torch.empty(M, Lp["proj"].k, dtype=cd, device=dev)
            Lp["proj"].dgrad(t, dao_op)
            dao = dao_op[:, :D] if "proj" in SL else dao_op
            if "proj" in SL:
                xdp, maskp = SL["proj"]
                self._site_backward(blk.attn.proj, Lp["at_proj"], S["ao_op"][:, D:D + R_PAD], t, dao_op[:, D:D + R_PAD], dao,
                                    xdp if xdp is not None else S["ao"], maskp, grads, g0 + gidx["proj"])
            dqkv = DQKVall[li] if wg_batched else torch.empty(M, 3 * D, dtype=cd, device=dev)
            qkv = S["qkv"]
            ops.attn_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], S["ao"], S["lse"], dao, dqkv[:, :D], dqkv[:, D:2 * D],
                         dqkv[:, 2 * D:], nimg, H, hd, Np, 1, Np, 1, scale)
            kq = Lp["qkv"].k
            da1 = DA1all[li] if wg_batched else torch.empty(M, kq, dtype=cd, device=dev)
            Lp["qkv"].dgrad(dqkv, da1)
            if isinstance(q, LoraLinear) and wg_batched:
                # d LN1(x) = da1[:, :D] + mask * (s * dT @ A); the weight gradients of this layer wait for their batch
                ep = dict(ep_mode=ops.EP_MUL, aux=S["mask"]) if S["mask"] is not None else {}
                ops.gemm(da1[:, D:D + R_PAD], Lp["at"], da1[:, :D], alpha=q.scaling, residual=da1[:, :D], **ep)
            elif isinstance(q, LoraLinear):
                a1 = S["a1"]
                self._site_backward(q, Lp["at"], a1[:, D:D + R_PAD], dqkv, da1[:, D:D + R_PAD], da1[:, :D],
                                    S["xd"] if S["xd"] is not None else a1[:, :D], S["mask"], grads, g0 + gidx["qkv"])
            if fuse_t1 and li > 0:  # dx becomes d(x_out) of block li-1: its tap gradient goes in first, then LN1 backward
                add_tap(li - 1)     # accumulates and emits t = bf16(dx * g2[li-1]) for that block's fc2 dgrad
                ops.layernorm_bwd_scaled(da1[:, :D], S["x_in"], Lp["n1w"], S["st1"], dx, t, P["layers"][li - 1]["g2"],
                                         accumulate_dx=True)
            else:
                ops.layernorm_bwd(da1[:, :D], S["x_in"], Lp["n1w"], S["st1"], dx, accumulate_dx=True)
                t = None
            ctx["saved"][li] = None
            if wg_batched:
                if li == half or li == 0:
                    lo, hi = (half, nL) if li == half and half > 0 else (0, half if half > 0 else nL)
                    self._lora_wgrads_batched(P, ctx, DA1all, DQKVall, lo, hi, M, D)
                    if BACKWARD_EVENTS["block_done"] is not None:
                        for lj in range(hi - 1, lo - 1, -1):
                            BACKWARD_EVENTS["block_done"](lj)
            elif BACKWARD_EVENTS["block_done"] is not None:
                BACKWARD_EVENTS["block_done"](li)
        if rein is not None:
            grads += self._rein_backward_end(rein, rein_acc)
        return grads

    @staticmethod
    def _site_backward(q, at_op, T, dy, dT, dxv, xd, mul, grads, gi):
        """One adapted site of one layer, after the dgrad GEMM d[x | T] = dy [W | B] wrote dxv = d x (base part) and dT:
        the factor gradients dB^T[r, out] = T^T dy and dA[r, in] = s dT^T drop(x) (reductions over the M tokens; `xd` = drop(x), or x itself
        without dropout) - into the optimiser's flat buffer where there is one, else grads[gi] / grads[gi + 1] - and then
        dxv += mul * (s dT A) in place (`mul`: the dropout multiplier, None without dropout; fc2 passes gelu'(pre) [* mask])."""
        from .functional import direct_grad_target
        r = q.r
        A, Bm = q.lora_A["default"].weight, q.lora_B["default"].weight
        dev = dy.device
        tB, tA = direct_grad_target(Bm), direct_grad_target(A)
        gBt = torch.empty(R_PAD, Bm.shape[0], dtype=torch.float32, device=dev)
        gAp = torch.empty(R_PAD, A.shape[1], dtype=torch.float32, device=dev)
        # with a flat gradient buffer the split-K combine scatters straight into B.grad [out, r] / A.grad [r, in]
        doneB = _wgrad_small_t(T, dy, gBt, scatter=None if tB is None else (tB, r, 1, r))
        doneA = _wgrad_small_t(dT, xd, gAp, alpha=q.scaling, scatter=None if tA is None else (tA, r, A.shape[1], 1))
        if doneB is True:
            pass
        elif tB is not None:
            ops.strided_copy(gBt, tB, (Bm.shape[0], r), (1, gBt.stride(0)), (r, 1), accumulate=True)
        else:
            gB = torch.empty_like(Bm, dtype=torch.float32)
            ops.strided_copy(gBt, gB, (Bm.shape[0], r), (1, gBt.stride(0)), (r, 1))
            grads[gi + 1] = gB
        if doneA is True:
            pass
        elif tA is not None:
            ops.axpby(gAp[:r].reshape(-1), 1.0, tA.view(-1), 1.0)
        else:
            grads[gi] = gAp[:r]
        ep = dict(ep_mode=ops.EP_MUL, aux=mul) if mul is not None else {}
        ops.gemm(dT, at_op, dxv, alpha=q.scaling, residual=dxv, **ep)

    # ---- full fine-tuning: d(xcat) -> gradients of full_params(), in that order (None where they went into the flat buffer)
    @staticmethod
    def _wgrad_full(dy, x, out):
        """out[N, K] += dy^T @ x over the token rows (dy [M, N], x [M, K] token-major, consumed in place; `out` a contiguous fp32 view -
        the parameter's slice of the optimiser's flat gradient buffer).  16-bit: the transposed-operand MFMA GEMM (GEMM_ATBT) with the
        accumulation in its epilogue; VFMSEG_FULL_WGRAD_SPLITK = k > 1 cuts the token reduction into k slabs (gemm_splitk_tn) that meet in
        a fixed order (slab_reduce) - more blocks for the 64-tile gradients, one more pass over k fp32 images.
        f32: strided operands.  Deterministic either way."""
        M, N = dy.shape
        K = x.shape[1]
        if not is_half(dy.dtype):
            ops.gemm(dy, x, out, residual=out, trans_a=True, trans_b=True)
            return
        if N % 8 or K % 8:
            wgrad(dy, x, out)      # (a patch size whose 3 P^2 is no multiple of 8: explicit transposes)
            return
        kch = int(os.environ.get("VFMSEG_FULL_WGRAD_SPLITK", "1"))
        steps = (M + 63) // 64
        if kch > 1 and steps % kch == 0 and dy.data_ptr() % 16 == 0 and dy.stride(0) % 8 == 0:
            slabs = torch.empty(kch, N, K, dtype=torch.float32, device=dy.device)
            ops.gemm_splitk_tn(dy, x, slabs, kch)
            ops.slab_reduce(slabs, N, out, K, 1, accumulate=True)
            return
        ops.gemm_tn_batched(dy.unsqueeze(0), x.unsqueeze(0), out.unsqueeze(0), M, accumulate=True)

    def _backward_full(self, ctx, dxcat):
        """The block backward of backward() plus every parameter gradient of the base: per block, last to first,
            dW_fc2 += t^T g, (d ls2.gamma, db_fc2, t = cd(dx g2)) from ONE pass (ops.branch_param_grads), dW_fc1 += dh^T a2, db_fc1,
            LayerNorm-2 dw / db, dW_proj += t^T ao, (d ls1.gamma, db_proj, t), dW_qkv += dqkv^T a1, db_qkv, LayerNorm-1 dw / db,
        then d pos_embed (token-row gradients summed over the images, class row included), d cls_token, dW_pe = dptok^T A0, db_pe.
        Gradients accumulate straight into the optimiser's flat buffer where there is one.  block_done(li) fires when block li's
        gradients are final, i.e. after its LayerNorm-1 backward."""
        from .functional import direct_grad_target
        v, P = self.vit, ctx["P"]
        cd, dev = P["cd"], P["dev"]
        D, H = v.embed_dim, v.num_heads
        hd = D // H
        scale = hd ** -0.5
        M, Mp, nimg, Np = ctx["M"], ctx["Mp"], ctx["nimg"], ctx["Np"]
        params = self.full_params()
        tgt, ret = {}, {}

        def G(p):
            """fp32 accumulator of p's gradient, flat: the flat-buffer slice, or a zeroed tensor that is handed to autograd"""
            if p is None:
                return None
            k = id(p)
            if k not in tgt:
                t_ = direct_grad_target(p)
                if t_ is None:
                    t_ = ret[k] = torch.zeros(p.shape, dtype=torch.float32, device=dev)
                tgt[k] = t_
            return tgt[k].view(-1)

        def G2(p):
            return G(p).view(p.shape[0], -1)

        dx = torch.zeros(M, D, dtype=torch.float32, device=dev)
        t = torch.empty(M, D, dtype=cd, device=dev)
        for li in range(len(v.blocks) - 1, -1, -1):
            blk, Lp, S = v.blocks[li], P["layers"][li], ctx["saved"][li]
            for i, oi in enumerate(v.out_indices):   # dx is d(x_out) of this block: its tap gradients go in first
                if oi == li:
                    src = dxcat[:, i * D:(i + 1) * D]
                    ops.strided_copy(src, dx, (Mp, D), (src.stride(0), 1), (D, 1), accumulate=True)
            # ---- MLP branch: x_out = x_mid + g2 * (fc2(gelu(fc1(LN2(x_mid)))) + b)
            fc1, fc2 = blk.mlp.fc1, blk.mlp.fc2
            ops.branch_param_grads(dx, S["u2"], Lp["g2"], dgamma=G(blk.ls2.gamma), dbias=G(fc2.bias), t=t, accumulate=True)
            self._wgrad_full(t, S["g"], G2(fc2.weight))
            hid = Lp["fc1"].n
            dh = ops.empty_ld(M, hid, cd, dev)
            Lp["fc2"].dgrad(t, dh, ep_mode=ops.EP_MUL, aux=S["hpre"])
            self._wgrad_full(dh, S["a2"], G2(fc1.weight))
            if fc1.bias is not None:
                ops.colsum(dh, G(fc1.bias), accumulate=True)
            dn = torch.empty(M, D, dtype=cd, device=dev)
            Lp["fc1"].dgrad(dh, dn)
            del dh
            ops.layernorm_bwd(dn, S["x_mid"], Lp["n2w"], S["st2"], dx, accumulate_dx=True, dw=G(blk.norm2.weight), db=G(blk.norm2.bias))
            # ---- attention branch: x_mid = x_in + g1 * (proj(attn(qkv(LN1(x_in)))) + b)
            qkv_l, proj = blk.attn.qkv, blk.attn.proj
            ops.branch_param_grads(dx, S["u1"], Lp["g1"], dgamma=G(blk.ls1.gamma), dbias=G(proj.bias), t=t, accumulate=True)
            self._wgrad_full(t, S["ao"], G2(proj.weight))
            dao = dn
            Lp["proj"].dgrad(t, dao)
            dqkv = torch.empty(M, 3 * D, dtype=cd, device=dev)
            qkv = S["qkv"]
            ops.attn_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], S["ao"], S["lse"], dao, dqkv[:, :D], dqkv[:, D:2 * D],
                         dqkv[:, 2 * D:], nimg, H, hd, Np, 1, Np, 1, scale)
            self._wgrad_full(dqkv, S["a1"], G2(qkv_l.weight))
            if qkv_l.bias is not None:
                ops.colsum(dqkv, G(qkv_l.bias), accumulate=True)
            da1 = torch.empty(M, D, dtype=cd, device=dev)
            Lp["qkv"].dgrad(dqkv, da1)
            ops.layernorm_bwd(da1, S["x_in"], Lp["n1w"], S["st1"], dx, accumulate_dx=True, dw=G(blk.norm1.weight), db=G(blk.norm1.bias))
            ctx["saved"][li] = None
            if BACKWARD_EVENTS["block_done"] is not None:
                BACKWARD_EVENTS["block_done"](li)
        # ---- embeddings: x0[patch j of image i] = ptok + pos[1 + j], x0[class row i] = cls + pos[0]
        gpos = G(v.pos_embed).view(Np + 1, D)
        for i in range(nimg):
            ops.strided_copy(dx[i * Np:(i + 1) * Np], gpos[1:], (Np, D), (D, 1), (D, 1), accumulate=True)
        ops.colsum(dx[Mp:], gpos[0], accumulate=True)
        ops.colsum(dx[Mp:], G(v.cls_token), accumulate=True)
        pe = v.patch_embed.proj
        if pe.bias is not None:
            ops.colsum(dx[:Mp], G(pe.bias), accumulate=True)
        if cd == torch.float32:
            dptok = dx[:Mp]
        else:
            dptok = torch.empty(Mp, D, dtype=cd, device=dev)
            ops.cast(dx[:Mp], dptok)
        self._wgrad_full(dptok, ctx["A0"], G2(pe.weight))
        ctx["A0"] = None
        return [ret.get(id(p)) for p in params]

    # ---- Rein adapter (reins.py:84-116): x' = x + scale * mlp_delta_f(softmax(c x T^T)[:, 1:] V + x) on the patch rows
    def _rein_fused(self, P):
        """The token attention of the adapter step has two forms with the same arithmetic: the composed one (ops.gemm + ops.softmax_rows +
        ops.cast: the project's tuned GEMMs, four launches per direction) and the fused kernels (vfm_rein_mix_fwd / _bwd: one launch, the score and
        probability maps never leave the chip).  VFMSEG_REIN_FUSED=1 selects the fused kernels in the 16-bit modes for the shapes they cover
        (D % 256 == 0, token_length <= 128); the default is the composed form, which measures faster in both directions at 2048 and at
        9216 rows - the exact-fp32 and split-bf16 modes always take it (ops.gemm gives their products)."""
        r = self.vit.reins
        return (is_half(P["cd"]) and os.environ.get("VFMSEG_REIN_FUSED", "0") == "1" and self.vit.embed_dim % 256 == 0
                and r.token_length <= ops.REIN_TOK)

    def _rein_pack(self, P):
        """Per forward call (the parameters move every optimiser step): the tokens T_l = A_l B_l and the values V_l = T_l[1:] W_t2f^T + b of
        ALL layers as [L, TP, D] operands in the compute dtype with zero pad rows (V with a zero row 0: column 0 of the softmax attends to
        nothing), their transposes for the fused kernels, mlp_delta_f packed, and `scale` spread over a D-vector for the GEMM epilogue."""
        from .optim import PARAM_EPOCH
        r = self.vit.reins
        cd, dev = P["cd"], P["dev"]
        D, nL, m = self.vit.embed_dim, r.num_layers, r.token_length
        live = r.live_params()
        key = (PARAM_EPOCH[0], self._rein_fused(P)) + tuple(x for p_ in live for x in (p_._version, p_.data_ptr()))
        R = P.get("rein")
        if R is not None and R["key"] == key:
            return R
        TP = (max(m, ops.REIN_TOK) + 63) // 64 * 64
        if R is None or R["TP"] != TP:
            z = lambda *sh, dt=cd: torch.zeros(*sh, dtype=dt, device=dev)   # noqa: E731  (pad rows are written once, here)
            R = P["rein"] = dict(TP=TP, T32=z(nL, TP, D, dt=torch.float32), T=z(nL, TP, D), V=z(nL, TP, D), TT=None, VT=None,
                                 scalevec=torch.empty(D, dtype=torch.float32, device=dev))
        R["key"], R["m"], R["c"], R["fused"] = key, m, float(D) ** -0.5, self._rein_fused(P)
        with torch.no_grad():
            T32 = R["T32"]
            toks = [p_.detach() for p_ in r.token_params()]
            if len(toks) == 2:   # LoRAReins: T_l = A_l @ B_l (exact fp32, K = lora_dim)
                ops.gemm(toks[0], toks[1], T32[:, :m], trans_b=True)
            else:
                ops.strided_copy(toks[0], T32, (nL, m, D), (m * D, D, 1), (TP * D, D, 1))
            if cd != torch.float32:
                ops.cast(T32.view(nL * TP, D), R["T"].view(nL * TP, D))
            else:
                R["T"] = T32
            Wt, Wd = r.mlp_token2feat, r.mlp_delta_f
            R["wt"], R["wd"] = Packed(Wt.weight.detach(), cd), Packed(Wd.weight.detach(), cd)
            R["bt"], R["bd"] = Wt.bias.detach(), Wd.bias.detach()
            vtmp = torch.empty(nL * TP, D, dtype=torch.float32, device=dev)
            R["wt"].fwd(R["T"].view(nL * TP, D), vtmp, bias=R["bt"])
            vt3 = vtmp.view(nL, TP, D)
            ops.strided_copy(vt3[:, 1:m], R["V"][:, 1:m], (nL, m - 1, D), (TP * D, D, 1), (TP * D, D, 1))
            if R["fused"]:
                if R["TT"] is None:
                    R["TT"], R["VT"] = torch.zeros(nL, D, TP, dtype=cd, device=dev), torch.zeros(nL, D, TP, dtype=cd, device=dev)
                ops.strided_copy(T32, R["TT"], (nL, D, m), (TP * D, 1, D), (D * TP, TP, 1))
                ops.strided_copy(vt3[:, 1:m], R["VT"][:, :, 1:m], (nL, D, m - 1), (TP * D, 1, D), (D * TP, TP, 1))
            ops.strided_copy(r.scale.detach().reshape(1), R["scalevec"], (D,), (0,), (1,))
        return R

    def _rein_forward(self, R, li, x, Mp, S):
        """x [M, D] fp32 stream after block li -> the stream after the adapter.  S (training with gradients): the dict backward reads; the
        stream is then NOT updated in place (the block's own backward and the token gradient dT = dS^T x read the pre-adapter rows)."""
        cd, dev = R["T"].dtype, x.device
        D, m, TP = x.shape[1], R["m"], R["TP"]
        xp = x[:Mp]
        u = torch.empty(Mp, D, dtype=cd, device=dev)
        p = torch.empty(Mp, TP, dtype=cd, device=dev) if S is not None else None
        x16 = None
        if R["fused"]:
            x16 = torch.empty(Mp, D, dtype=cd, device=dev) if S is not None else None
            ops.rein_mix_fwd(xp, R["T"][li], R["VT"][li], u, m, R["c"], p=p, x16=x16)
        else:
            if cd != torch.float32:
                x16 = torch.empty(Mp, D, dtype=cd, device=dev)
                ops.cast(xp, x16)
            sc = torch.empty(Mp, TP, dtype=torch.float32, device=dev)
            ops.gemm(x16 if x16 is not None else xp, R["T"][li], sc, alpha=R["c"])
            if p is None:
                p = torch.empty(Mp, TP, dtype=cd, device=dev)
            ops.softmax_rows(sc, p, m)
            ops.gemm(p, R["V"][li], u, residual=xp, trans_b=True)
        if S is None:
            xn = x     # nothing reads the pre-adapter rows again: the epilogue's residual is its own destination
        else:
            xn = torch.empty_like(x)
            ops.cast(x[Mp:], xn[Mp:])   # the class tokens pass through
            S.update(rein_u=u, rein_p=p, rein_x=x16 if x16 is not None else xp)
        R["wd"].fwd(u, xn[:Mp], bias=R["bd"], colscale=R["scalevec"], residual=xp)
        return xn

    def _rein_backward_begin(self, R):
        dev = R["T"].device
        nL, TP, D = R["T"].shape
        z = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=dev)   # noqa: E731
        return dict(dT=z(nL, TP, D), dV=z(nL, TP, D), Gm=z(D, D), gb=z(D))

    @staticmethod
    def _tn(xs, y, out, alpha=1.0, accumulate=False):
        """out[P, Q] (+)= alpha * xs^T @ y over the token rows, both operands consumed token-major."""
        if is_half(xs.dtype):
            ops.gemm_tn_batched(xs.unsqueeze(0), y.unsqueeze(0), out.unsqueeze(0), xs.shape[0], alpha=alpha, accumulate=accumulate)
        else:
            ops.gemm(xs, y, out, alpha=alpha, residual=out if accumulate else None, trans_a=True, trans_b=True)

    def _rein_backward(self, R, acc, li, dx, Mp, S):
        """dx[:Mp] holds d x' of layer li's adapter (tap gradient included) and becomes d x; the token / value gradients of the layer and
        the running sums of the shared mlp_delta_f gradients go to `acc` (ISSUE formulas: reins.py:84-116 under autograd)."""
        cd, dev = R["T"].dtype, dx.device
        D, m, TP, c = dx.shape[1], R["m"], R["TP"], R["c"]
        u, p, xs = S["rein_u"], S["rein_p"], S["rein_x"]
        g = torch.empty(Mp, D, dtype=cd, device=dev)
        ops.cast(dx[:Mp], g)
        # shared mlp_delta_f: Gm += g^T u and gb += colsum(g) (the learnable scale multiplies them at the end, and gives dscale)
        self._tn(g, u, acc["Gm"], accumulate=True)
        ops.colsum(g, acc["gb"], accumulate=True)
        du = torch.empty(Mp, D, dtype=cd, device=dev)
        R["wd"].dgrad(g, du, colscale=R["scalevec"])          # du = (scale g) W_d
        ds = torch.empty(Mp, TP, dtype=cd, device=dev)
        if R["fused"]:
            ops.rein_mix_bwd(du, p, R["V"][li], R["TT"][li], ds, dx[:Mp], m, c)
            a = 1.0
        else:
            dp = torch.empty(Mp, TP, dtype=torch.float32, device=dev)
            ops.gemm(du, R["V"][li], dp)                        # column 0 and the pad columns meet zero rows of V
            ops.softmax_rows_bwd(p, dp, ds, m, 1, 1)
            ops.gemm(ds, R["T"][li], dx[:Mp], alpha=c, residual=dx[:Mp], trans_b=True)
            ops.strided_copy(du, dx[:Mp], (Mp, D), (du.stride(0), 1), (dx.stride(0), 1), accumulate=True)
            a = c
        self._tn(ds, xs, acc["dT"][li], alpha=a)               # dT = dS^T x
        self._tn(p, du, acc["dV"][li])                         # dV = P^T du (row 0 is dropped at the end)
        S["rein_u"] = S["rein_p"] = S["rein_x"] = None

    def _rein_backward_end(self, R, acc):
        """The layer-batched tail: dT[1:] += dV W_t2f, the token-factor gradients, mlp_token2feat's and mlp_delta_f's gradients, dscale.
        Gradients go straight into the optimiser's flat buffer where it exposes one (None is handed to autograd then)."""
        from .functional import direct_grad_target
        r = self.vit.reins
        cd, dev = R["T"].dtype, R["T"].device
        nL, TP, D = R["T"].shape
        m = R["m"]
        z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device=dev)   # noqa: E731
        # dV with row 0 and the pad rows dropped, in the compute dtype
        dvz = z(nL, TP, D, dt=cd)
        ops.strided_copy(acc["dV"][:, 1:m], dvz[:, 1:m], (nL, m - 1, D), (TP * D, D, 1), (TP * D, D, 1))
        dvz2, T2 = dvz.view(nL * TP, D), R["T"].view(nL * TP, D)
        gWt, gbt = z(D, D), z(D)
        self._tn(dvz2, T2, gWt)                                 # dW_t2f = dV^T T[1:] (row 0 of dvz is zero)
        ops.colsum(dvz2, gbt)
        back = torch.empty(nL * TP, D, dtype=torch.float32, device=dev)
        R["wt"].dgrad(dvz2, back)                               # dV W_t2f
        dT = acc["dT"]
        ops.strided_copy(back.view(nL, TP, D)[:, 1:m], dT[:, 1:m], (nL, m - 1, D), (TP * D, D, 1), (TP * D, D, 1), accumulate=True)
        toks = r.token_params()
        if len(toks) == 2:
            A, Bm = toks[0].detach(), toks[1].detach()
            gA, gB = torch.empty_like(A), torch.empty_like(Bm)
            ops.gemm(dT[:, :m], Bm, gA)                          # dA_l = dT_l B_l^T
            ops.gemm(A, dT[:, :m], gB, trans_a=True, trans_b=True)   # dB_l = A_l^T dT_l
            gtok = [gA, gB]
        else:
            gt = torch.empty_like(toks[0])
            ops.strided_copy(dT, gt, (nL, m, D), (TP * D, D, 1), (m * D, D, 1))
            gtok = [gt]
        # dscale = <sum_l g^T u, W_d> + <sum_l colsum g, b_d>; then dW_d = scale * Gm, db_d = scale * gb
        Gm, gb = acc["Gm"], acc["gb"]
        prod = torch.empty(D, D, dtype=torch.float32, device=dev)
        ops.mul_mask(Gm, r.mlp_delta_f.weight.detach(), prod)
        part = torch.empty(D, dtype=torch.float32, device=dev)
        ops.colsum(prod, part)
        pb = torch.empty(1, D, dtype=torch.float32, device=dev)
        ops.mul_mask(gb.view(1, D), R["bd"].view(1, D), pb)
        ops.axpby(pb.view(-1), 1.0, part, 1.0)
        gscale = z(1)
        ops.colsum(part.view(D, 1), gscale)
        ops.scale_by_device_scalar(Gm.view(-1), r.scale.detach())
        ops.scale_by_device_scalar(gb, r.scale.detach())
        out = []
        for p_, g_ in zip(r.live_params(), gtok + [gWt, gbt, Gm, gb, gscale.view(())]):
            tgt = direct_grad_target(p_)
            if tgt is not None:
                ops.axpby(g_.reshape(-1), 1.0, tgt.view(-1), 1.0)
                out.append(None)
            else:
                out.append(g_)
        return out

    def _lora_wgrads_batched(self, P, ctx, DA1all, DQKVall, lo, hi, M, D):
        """LoRA weight gradients of layers [lo, hi): two batched TN GEMMs + one batched scatter-accumulate into the flat buffer."""
        from .functional import direct_grad_target
        v = self.vit
        n = hi - lo
        dev = DA1all.device
        ws = P.setdefault("wg_ws", {})
        key = (lo, hi, M)
        w = ws.get(key)
        # dA has only D / 128 output tiles per layer (its 64 rows are one tile row): n * 8 = 96 blocks for 256 CUs.  The token
        # reduction is therefore cut into `ksp` equal row ranges that run as batch entries of their own (each layer's rows are
        # contiguous, so range c of layer l is entry ksp * l + c of ONE strided batch) and meet in the scatter-accumulate below.
        ksp = 4 if (M % 4 == 0 and n * (D // 128) * 4 <= 512) else (2 if (M % 2 == 0 and n * (D // 128) * 2 <= 512) else 1)
        if os.environ.get("VFMSEG_LORA_WGRAD_KSPLIT", "1") == "0":
            ksp = 1
        if w is None:
            w = ws[key] = dict(outB=torch.empty(n, R_PAD, 3 * D, dtype=torch.float32, device=dev),
                               outA=torch.empty(n * ksp, R_PAD, D, dtype=torch.float32, device=dev), table=None, sig=None)
        A1all, XDall = ctx["A1all"], ctx["XDall"]
        q0 = v.blocks[lo].attn.qkv
        ops.gemm_tn_batched(A1all[lo:hi, :, D:D + R_PAD], DQKVall[lo:hi], w["outB"], M)                       # dB^T = T^T dqkv
        Y = XDall[lo:hi] if XDall is not None else A1all[lo:hi, :, :D]
        dT = DA1all[lo:hi, :, D:D + R_PAD]
        if ksp > 1:
            mk = M // ksp
            dT = dT.as_strided((n * ksp, mk, R_PAD), (mk * dT.stride(1), dT.stride(1), 1), dT.storage_offset())
            Y = Y.as_strided((n * ksp, mk, D), (mk * Y.stride(1), Y.stride(1), 1), Y.storage_offset())
            ops.gemm_tn_batched(dT, Y, w["outA"], mk, alpha=q0.scaling)                                       # dA = s dT^T drop(LN x)
        else:
            ops.gemm_tn_batched(dT, Y, w["outA"], M, alpha=q0.scaling)
        tg = []
        for l in range(lo, hi):
            q = v.blocks[l].attn.qkv
            tg.append((direct_grad_target(q.lora_A["default"].weight), direct_grad_target(q.lora_B["default"].weight), q.r))
        sig = tuple((a.data_ptr(), b.data_ptr()) for a, b, _ in tg) + (ksp,)
        if w["table"] is None or w["sig"] != sig:
            jobs = []
            for i, (tA, tB, r) in enumerate(tg):
                jobs.append((w["outB"][i], tB, (3 * D, r), (1, 3 * D), (r, 1), True))     # B.grad[n, rr] += outB[rr, n]
                # A.grad[rr, k] += sum over the ksp token ranges of outA[rr, k] (ONE job: jobs of a table run concurrently)
                jobs.append((w["outA"][i * ksp], tA, (r, D), (D, 1), (D, 1), True, ksp, R_PAD * D))
            w["table"], w["sig"] = ops.CopyBatch(jobs), sig
        w["table"].run()


def _refresh_sites(P, sites):
    """sites: (A, B, a, at, w, wt, r, K, N, Kw) per adapter; fp32 contiguous parameters go through the batched pack kernel."""
    if not sites:
        return
    with torch.no_grad():
        if all(s_[0].dtype == torch.float32 and s_[0].is_contiguous() and s_[1].dtype == torch.float32 and s_[1].is_contiguous() for s_ in sites):
            tab = P.get("lora_table")
            if tab is None or not tab.valid_for(sites):
                tab = P["lora_table"] = ops.LoraPackTable(sites, sites[0][2])
            tab.run()
            return
        for (A, Bm, a, at, w, wt, r, K, N, Kw) in sites:
            ops.cast(A, a[:r])
            _pack_at(A, at, r)
            ops.cast(Bm, w[:, Kw:Kw + r])
            if wt is not None:
                ops.transpose(Bm, wt[Kw:Kw + r], pad_rows=Bm.shape[0])


def _pack_at(A, at, r):
    """at[:, :r] = A^T  (A [r, in])"""
    ops.strided_copy(A, at, (A.shape[1], r), (1, A.stride(0)), (at.stride(0), 1))


_KCH_MAX = int(os.environ.get("VFMSEG_WGRAD_KCH_MAX", "16"))


def _wgrad_small_t(xs, y, out, alpha=1.0, scatter=None):
    """out[P, Q] = alpha * xs^T @ y   with xs [M, P] small (P <= 64) and y [M, Q] large, consumed in place.
    bf16: only the small operand is transposed (zero-padded to a multiple of 64 tokens); the large one is the
    transposed-B operand of the MFMA GEMM.  f32: strided operands.
    scatter = (dst, rows_used, sp, sq): instead of writing `out`, accumulate dst[p*sp + q*sq] += result[p, q] for
    p < rows_used (the gradient's own layout inside the optimiser's flat buffer); returns True when that was done."""
    M = xs.shape[0]
    if is_half(xs.dtype):
        mp = (M + 63) // 64 * 64
        # few output tiles, long token reduction: split K into the largest divisor <= 16 of the 64-token steps
        steps = mp // 64
        kch = max(d for d in range(1, _KCH_MAX + 1) if steps % d == 0)
        tn = kch > 1 and xs.shape[1] % 8 == 0 and xs.data_ptr() % 16 == 0 and xs.stride(0) % 8 == 0
        if not tn:
            xt = torch.empty(xs.shape[1], mp, dtype=xs.dtype, device=xs.device)
            ops.transpose(xs, xt, pad_rows=mp)
        if kch > 1:
            P, Q = xs.shape[1], y.shape[1]
            slabs = torch.empty(kch, P, Q, dtype=torch.float32, device=xs.device)
            if tn:
                ops.gemm_splitk_tn(xs, y, slabs, kch)      # both operands token-major, consumed in place (no transposes)
            else:
                ops.gemm_splitk_bt(xt, y, slabs, kch)
            if scatter is not None:
                dst, rows_used, sp, sq = scatter
                ops.slab_reduce(slabs, rows_used, dst, sp, sq, alpha=alpha, accumulate=True)
                return True
            ops.colsum(slabs.view(kch, P * Q), out.view(P * Q))
            if alpha != 1.0:
                ops.axpby(out.view(-1), alpha, out.view(-1), 0.0)
        else:
            ops.gemm(xt, y, out, alpha=alpha, trans_b=True, kb_rows=M)
    else:
        ops.gemm(xs, y, out, alpha=alpha, trans_a=True, trans_b=True)
    return out


class _BackboneFn(torch.autograd.Function):
    """One autograd node for the whole ViT: forward saves activations, backward runs the hand-written block backward."""

    @staticmethod
    def forward(ctx, vit, jobs, training, seed, *lora_params):
        eng = vit.engine()
        need_grad = training and any(p.requires_grad for p in lora_params)
        with ops.region("backbone"):
            if isinstance(eng, DinoEngine):
                xcat, grid, c = eng.forward(jobs, training, seed, need_grad=need_grad)
            else:
                xcat, grid, c = eng.forward(jobs, training, seed)
        if need_grad:
            ctx.eng, ctx.c = eng, c
            _PENDING_BACKWARD[0] += 1
        else:
            c["saved"] = None
        ctx.nparams = len(lora_params)
        ctx.mark_non_differentiable()
        ctx.set_materialize_grads(False)
        ctx.grid = grid
        return xcat, _Grid(grid)

    @staticmethod
    def backward(ctx, dxcat, _):
        _PENDING_BACKWARD[0] = max(_PENDING_BACKWARD[0] - 1, 0)
        if dxcat is None:
            return (None, None, None, None) + (None,) * ctx.nparams
        if BACKWARD_EVENTS["heads_done"] is not None:
            from .functional import join_wgrad_stream
            join_wgrad_stream()     # (the heads' weight gradients run on a side stream; their DP buckets leave now)
            BACKWARD_EVENTS["heads_done"]()
        with ops.region("backbone"):
            grads = ctx.eng.backward(ctx.c, dxcat.contiguous())
        if BACKWARD_EVENTS.get("backbone_done") is not None and _PENDING_BACKWARD[0] == 0:
            BACKWARD_EVENTS["backbone_done"]()    # gradients shared by all layers (Rein) are complete only now
        return (None, None, None, None) + tuple(grads)


class _Grid(tuple):
    """(hp, wp) carried through autograd.Function as a non-tensor output."""
    pass
