"""Shared pieces of the full fine-tuning tests (tests/test_fullft_cpu.py, tests/test_fullft_gpu.py, tests/fullft_dp_worker.py).

The small model is the smallest at which every piece can still go wrong: depth 2, out_indices [0, 1, 1, 1] (a repeated tap),
embed_dim 256 with 4 heads, img_size 64 and batches of 64 x 64 images - 16 patch rows + 1 class row per image, M = 34 token rows at
batch 2: no multiple of 64, so the zero-row padding of the transposed GEMM, the class rows and the reductions' tails are all used.
The oracle is autograd over oracle.torch_ref.dinov2_forward(..., lora=False, p='backbone.') in float64 on the CPU."""
import functools

import torch

from oracle import torch_ref as R
from vfmseg_amd import presets
from vfmseg_amd.registry import MODELS
from vfmseg_amd.synth import synth_image, synth_label, synth_like

DEPTH, DIM, HEADS, IMG = 2, 256, 4, 64
OUT_IDX = [0, 1, 1, 1]
BB = "backbone."


def small_cfg(head="linear", kind="full"):
    """kind: 'full' (EncoderDecoder over the bare backbone) | 'frozen' (FrozenBackboneEncoderDecoder over the same backbone)."""
    make = presets.full_dinov2_linear if head == "linear" else presets.full_dinov2_segformer
    cfg = make(depth=DEPTH, embed_dim=DIM, num_heads=HEADS, img_size=IMG)
    cfg["backbone"]["out_indices"] = list(OUT_IDX)
    cfg["decode_head"]["dropout_ratio"] = 0.0
    if head == "linear":
        cfg["decode_head"]["channels"] = DIM // 4      # LinearHead's two 2x up-convolutions leave a quarter of the tap width
    cfg["test_cfg"] = dict(mode="whole")
    if kind == "frozen":
        cfg["type"] = "FrozenBackboneEncoderDecoder"
    return cfg


@functools.lru_cache(maxsize=None)
def _small_sd(head):
    return synth_like(MODELS.build(small_cfg(head)).state_dict())


def small_state_dict(head="linear"):
    """Synthetic weights of the small model (fresh clones of one cached dict)."""
    return {k: v.clone() for k, v in _small_sd(head).items()}


def build_small(head="linear", kind="full", sd=None):
    model = MODELS.build(small_cfg(head, kind))
    model.load_state_dict(small_state_dict(head) if sd is None else sd)
    return model


def trained_backbone_keys(sd):
    """Backbone keys that enter the graph (everything but the final norm and the mask token)."""
    return [k for k in sd if k.startswith(BB) and not k.startswith(BB + "norm.") and k != BB + "mask_token"]


def inert_backbone_keys(sd):
    return [k for k in sd if k.startswith(BB + "norm.") or k == BB + "mask_token"]


def batch(bs=2, seed=0):
    return synth_image(bs, IMG, seed=seed), synth_label(bs, IMG, seed=seed)


def oracle_taps(sd, img, dtype=torch.float64):
    """[B * Np, 4 * D] token-major taps (the layout of forward_tokens' xcat) from the oracle, in `dtype`; sd's tensors are used as they
    are (leaves of the caller's graph)."""
    outs = R.dinov2_forward(sd, img.to(dtype), depth=DEPTH, heads=HEADS, out_indices=tuple(sorted(set(OUT_IDX))), lora=False, p=BB)
    by_layer = dict(zip(sorted(set(OUT_IDX)), outs))
    cols = [by_layer[i].permute(0, 2, 3, 1).reshape(-1, DIM) for i in OUT_IDX]
    return torch.cat(cols, dim=1)


@functools.lru_cache(maxsize=None)
def oracle_backbone_grads(seed=0):
    """(taps, {key: d loss / d tensor}, R) for loss = sum(taps * R) with a fixed random R, float64; computed once and shared."""
    sd = {k: v.double() for k, v in small_state_dict().items()}
    keys = trained_backbone_keys(sd)
    for k in keys:
        sd[k].requires_grad_(True)
    img, _ = batch(2, seed)
    taps = oracle_taps(sd, img)
    Rw = torch.randn(taps.shape, generator=torch.Generator().manual_seed(77 + seed), dtype=torch.float64)
    grads = torch.autograd.grad((taps * Rw).sum(), [sd[k] for k in keys])
    return taps.detach(), dict(zip(keys, grads)), Rw


def oracle_train_steps(n_steps, optim_wrapper_cfg, end):
    """n_steps iterations of EncoderDecoder(bare DinoVisionTransformer, LinearHead) on the oracle in float64: forward (backbone taps,
    linear_head_forward in training mode, bilinear + CE), autograd, AdamW per parameter with the config's groups (param_options of the
    product gives lr_mult / decay per name; checked against the config in tests/test_fullft_cpu.py) at lr = PolyLR(t), the parameter
    itself kept in fp32 between the steps as the optimiser's master is.
    Returns (losses, state dict after the steps)."""
    from vfmseg_amd.optim import param_options
    model = build_small()
    model.train()
    oc = optim_wrapper_cfg["optimizer"]
    opts = param_options(model, oc["lr"], oc["weight_decay"], optim_wrapper_cfg.get("paramwise_cfg"))
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in small_state_dict().items()}
    state, losses = {}, []
    for t in range(n_steps):
        img, lab = batch(2, seed=40 + t)
        work = dict(sd)
        for k in opts:
            work[k] = sd[k].detach().clone().requires_grad_(True)
        taps = oracle_taps(work, img)
        B = img.shape[0]
        feats = [taps[:, i * DIM:(i + 1) * DIM].reshape(B, IMG // 16, IMG // 16, DIM).permute(0, 3, 1, 2) for i in range(len(OUT_IDX))]
        bn = {}
        logits = R.linear_head_forward(work, feats, training=True, bn_out=bn)
        loss, _, _ = R.head_loss(logits, lab)
        keys = list(opts)
        grads = torch.autograd.grad(loss, [work[k] for k in keys], allow_unused=True)
        losses.append(float(loss.detach()))
        sd["decode_head.output_upscaling.1.running_mean"] = bn["running_mean"].detach()
        sd["decode_head.output_upscaling.1.running_var"] = bn["running_var"].detach()
        lr_t = R.poly_lr(oc["lr"], t, end=end)
        with torch.no_grad():
            for k, g in zip(keys, grads):
                if g is None:
                    g = torch.zeros_like(sd[k])   # (the flat-buffer optimiser steps every trainable parameter: a zero gradient still decays)
                lr_mult, wd = opts[k]
                m, v = state.get(k, (torch.zeros_like(g), torch.zeros_like(g)))
                # torch.optim.AdamW on an fp32 parameter (what vfm_adamw restates) touches the parameter twice in fp32: param.mul_(1 - lr * wd)
                # with the factor rounded to fp32, and the store.  At lr_mult 0.1 three steps move a LayerScale gamma of magnitude 1 by ~2e-5,
                # ~200 ulps of its fp32 value: 1 - 5e-7 is 8.4 ulps below 1 and rounds to 8, a systematic 2.3e-8 p per step, and the store adds
                # up to half an ulp - together 2.2e-3 to 2.6e-3 of the update (measured on ls1 / ls2.gamma against the all-float64 step;
                # 3e-5 on tensors of small magnitude), for torch's own optimiser as for the fused one.  The oracle's step is therefore
                # evaluated with these two operations in the optimiser's format - the decay factor as an fp32 number, the parameter kept in
                # fp32 between steps - and everything else (moments, bias corrections, the Adam quotient) in float64 as adamw_step has it.
                lr_k = lr_t * lr_mult
                decay32 = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(lr_k, dtype=torch.float32) * torch.tensor(wd, dtype=torch.float32))
                p_new, m, v = R.adamw_step(sd[k].detach() * decay32, g, m, v, t + 1, lr_k, 0.0)
                sd[k] = p_new.float().double()
                state[k] = (m, v)
    return losses, sd
