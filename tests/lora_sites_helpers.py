"""Helpers of the LoRA adapter-site tests (no reference tree needed): the toy model of tests/golden/lora_sites.npz - DINOv2 width 1024,
depth 2, LoRA r = 8 on qkv, attn.proj, fc1 and fc2, batch 2 of 96 x 112 (a 6 x 7 token grid: 86 token rows) - its synthetic weights, and a
float64 restatement of the block with peft's lora.Linear on all four linear layers (oracle.torch_ref.lora_linear / attention).
tools/gen_lora_sites_golden.py uses the same recipe, so the fixture (written by the reference's own modules) and the tests see identical
parameters."""
import torch
import torch.nn.functional as F

from oracle import torch_ref as R
from vfmseg_amd import presets
from vfmseg_amd.synth import synth_image, synth_state_dict

ALL = ["qkv", "attn.proj", "fc1", "fc2"]
DEPTH, DIM, HEADS, RANK, ALPHA, OUT = 2, 1024, 16, 8, 32, (0, 1)
IMG_H, IMG_W, IMG_SEED, TAP_GRAD_SEED = 96, 112, 61, 17
HP, WP = IMG_H // 16, IMG_W // 16
PRE = "model.base_model.model."          # LoRABackbone -> PeftModel -> base_model.model
SITE_MODULE = {"qkv": "attn.qkv", "attn.proj": "attn.proj", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}


def backbone_cfg():
    return dict(presets.dinov2_backbone(depth=DEPTH), out_indices=list(OUT))


def lora_backbone_cfg(targets=ALL, dropout=0.0, r=RANK):
    return dict(type="LoRABackbone", backbone=backbone_cfg(), Lora_config=presets.lora_cfg(r=r, alpha=ALPHA, target_modules=list(targets), dropout=dropout))


def base_shapes(dim=DIM, depth=DEPTH, n_pos=1025):
    """bare DinoVisionTransformer state_dict (what a pretrained checkpoint holds)"""
    s = {"cls_token": (1, 1, dim), "pos_embed": (1, n_pos, dim), "mask_token": (1, dim), "patch_embed.proj.weight": (dim, 3, 16, 16),
         "patch_embed.proj.bias": (dim,), "norm.weight": (dim,), "norm.bias": (dim,)}
    for i in range(depth):
        q = f"blocks.{i}."
        for n in ("norm1", "norm2"):
            s[q + n + ".weight"], s[q + n + ".bias"] = (dim,), (dim,)
        s[q + "attn.qkv.weight"], s[q + "attn.qkv.bias"] = (3 * dim, dim), (3 * dim,)
        s[q + "attn.proj.weight"], s[q + "attn.proj.bias"] = (dim, dim), (dim,)
        s[q + "ls1.gamma"], s[q + "ls2.gamma"] = (dim,), (dim,)
        s[q + "mlp.fc1.weight"], s[q + "mlp.fc1.bias"] = (4 * dim, dim), (4 * dim,)
        s[q + "mlp.fc2.weight"], s[q + "mlp.fc2.bias"] = (dim, 4 * dim), (dim,)
    return s


def base_state_dict():
    return synth_state_dict(base_shapes())


def lora_state_dict(targets=ALL, r=RANK, dim=DIM, depth=DEPTH):
    """LoRABackbone.state_dict() of the toy model: the base under `.base_layer` where a module carries an adapter, non-zero factors."""
    wrapped = {SITE_MODULE[t] for t in targets}
    io = {"attn.qkv": (dim, 3 * dim), "attn.proj": (dim, dim), "mlp.fc1": (dim, 4 * dim), "mlp.fc2": (4 * dim, dim)}
    sd = {}
    for k, v in base_state_dict().items():
        mod, _, leaf = k.rpartition(".")
        tail = mod.split(".", 2)[2] if mod.startswith("blocks.") else None
        sd[PRE + (mod + ".base_layer." + leaf if tail in wrapped else k)] = v
    fac = {}
    for i in range(depth):
        for m in sorted(wrapped):
            fac[f"{PRE}blocks.{i}.{m}.lora_A.default.weight"] = (r, io[m][0])
            fac[f"{PRE}blocks.{i}.{m}.lora_B.default.weight"] = (io[m][1], r)
    sd.update(synth_state_dict(fac))   # (std 0.02 / 0.04 like every synthetic weight: B is not zero)
    return sd


def toy_image():
    return synth_image(2, (IMG_H, IMG_W), seed=IMG_SEED)


def tap_grads(dtype=torch.float32):
    """the seeded tap gradients of the fixture, NCHW per tap"""
    gen = torch.Generator().manual_seed(TAP_GRAD_SEED)
    return [torch.randn(2, DIM, HP, WP, generator=gen).to(dtype) for _ in OUT]


def dxcat_of(dts):
    """tap gradients (NCHW list) in the engine's token-major layout [2 * HP * WP, len(OUT) * DIM]"""
    return torch.stack([d.permute(0, 2, 3, 1) for d in dts], dim=3).reshape(2 * HP * WP, len(OUT) * DIM)


def taps_of(xcat):
    """the engine's xcat -> NCHW taps (CPU float64)"""
    v = xcat.detach().double().cpu().view(2, HP, WP, len(OUT), DIM)
    return [v[:, :, :, i].permute(0, 3, 1, 2) for i in range(len(OUT))]


def tap_grid(t):
    """a strided sample through the whole of a tap [2, DIM, HP, WP]: every 32nd channel at every position"""
    return t[:, 5::32]


def grad_grid(g):
    """a strided sample through the whole of a factor gradient ([r, in] or [out, r]): at most 8 x 64 elements spread over all rows / columns"""
    return g[::max(1, g.shape[0] // 64) if g.shape[0] > 8 else 1, ::max(1, g.shape[1] // 64) if g.shape[1] > 8 else 1]


def block_f64(sd, x, i, masks=None, p=PRE):
    """block.py:89-114 in the dtype of x with lora.Linear on all four linear layers; masks: {(layer, site module): already-scaled dropout
    multiplier [B, N, in]} or None."""
    q = f"{p}blocks.{i}."
    b, n, c = x.shape
    mk = lambda m: None if masks is None else masks.get((i, m))   # noqa: E731
    h = F.layer_norm(x, (c,), sd[q + "norm1.weight"], sd[q + "norm1.bias"], 1e-6)
    qkv = R.lora_linear(sd, q + "attn.qkv.", h, True, mk("attn.qkv")).reshape(b, n, 3, HEADS, c // HEADS).permute(2, 0, 3, 1, 4)
    o = R.attention(qkv[0], qkv[1], qkv[2], (c // HEADS) ** -0.5).transpose(1, 2).reshape(b, n, c)
    o = R.lora_linear(sd, q + "attn.proj.", o, True, mk("attn.proj"))
    x = x + o * sd[q + "ls1.gamma"]
    h = F.layer_norm(x, (c,), sd[q + "norm2.weight"], sd[q + "norm2.bias"], 1e-6)
    h = F.gelu(R.lora_linear(sd, q + "mlp.fc1.", h, True, mk("mlp.fc1")))
    h = R.lora_linear(sd, q + "mlp.fc2.", h, True, mk("mlp.fc2"))
    return x + h * sd[q + "ls2.gamma"]


def forward_f64(sd, img, masks=None, p=PRE):
    """the toy backbone in float64: NCHW taps.  sd: lora_state_dict() (tensors may require grad)."""
    sd = {k: (v.double() if torch.is_tensor(v) else v) for k, v in sd.items()}
    sd["__lora_scaling__"] = ALPHA / RANK
    img = img.double()
    t = R.dinov2_tokens(sd, img, 16, p)
    outs = []
    for i in range(DEPTH):
        t = block_f64(sd, t, i, masks, p)
        if i in OUT:
            outs.append(t[:, 1:].permute(0, 2, 1).reshape(img.shape[0], -1, HP, WP))
    return outs


def token_mask_to_bnc(mask, width):
    """an engine mask [M, width] (rows: the patch tokens image-major, then the [cls] tokens) -> [B, 1 + Np, width] in the reference's order"""
    Np = HP * WP
    m = mask.detach().double().cpu()
    return torch.cat([m[2 * Np:].view(2, 1, width), m[:2 * Np].view(2, Np, width)], dim=1)
