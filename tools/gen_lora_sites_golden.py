"""Writes tests/golden/lora_sites.npz from the REFERENCE's own modules (rein/models/backbones/dino_v2.py and lora_backbone.py, imported
through oracle/ref_shim.py; peft's lora.Linear as restated there): LoRA on qkv, attn.proj, fc1 and fc2 of a depth-2 DINOv2 of width 1024,
r = 8, dropout 0, batch 2 of 96 x 112.  Data only: tap slices, strided grids and statistics, gradient slices, strided grids and norms of
every factor, the sorted parameter names.  Runs where the reference tree exists; the tests read the .npz and tests/lora_sites_helpers.py only.

    python tools/gen_lora_sites_golden.py

The generator ASSERTS that switching off each site's adapter alone (its B = 0) moves every tap by >= 1 % of the tap's largest magnitude,
so a re-tuned recipe cannot make the fixture blind to a site."""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import lora_sites_helpers as H  # noqa: E402
from tests.helpers import sl, stats  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    torch.manual_seed(0)
    M = ref_shim.load_all()
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        torch.save(H.base_state_dict(), f.name)
        ck = f.name
    cfg = H.lora_backbone_cfg()
    cfg["checkpoint"] = ck
    model = M.build(cfg)
    os.unlink(ck)
    sd = H.lora_state_dict()
    have = model.state_dict()
    assert sorted(have) == sorted(sd), sorted(set(have) ^ set(sd))
    for k in have:   # the reference's own loader put the base weights under .base_layer (patch_embed.proj included, untouched)
        if "lora_" not in k:
            assert torch.equal(have[k], sd[k]), k
    model.load_state_dict(sd)
    model.train()     # LoRABackbone.train(): the base stays in eval; lora_dropout = 0
    x = H.toy_image()
    taps = model(x)
    assert len(taps) == len(H.OUT) and tuple(taps[0].shape) == (2, H.DIM, H.HP, H.WP), [t.shape for t in taps]
    out = {"param_names": np.array(sorted(have))}
    # sensitivity: each site's adapter off alone
    sens = np.zeros((len(H.ALL), len(taps)))
    named = dict(model.named_parameters())
    with torch.no_grad():
        for si, t_ in enumerate(H.ALL):
            keys = [k for k in named if "." + H.SITE_MODULE[t_] + ".lora_B." in k]
            assert len(keys) == H.DEPTH, keys
            keep = {k: named[k].data.clone() for k in keys}
            for k in keys:
                named[k].data.zero_()
            off = model(x)
            for k in keys:
                named[k].data.copy_(keep[k])
            sens[si] = [((a - b).abs().max() / a.abs().max()).item() for a, b in zip(taps, off)]
    assert (sens >= 0.01).all(), sens
    out["site_sensitivity"] = sens          # [site, tap] in units of the tap's max |x|
    loss = 0
    for i, (t, d) in enumerate(zip(taps, H.tap_grads())):
        out[f"tap{i}_stats"], out[f"tap{i}_slice"], out[f"tap{i}_tail"] = stats(t), sl(t), t.detach()[1, -5:, -3:, -4:].numpy().copy()
        out[f"tap{i}_grid"] = H.tap_grid(t.detach()).numpy().copy()
        loss = loss + (t * d).sum()
    loss.backward()
    trainable = []
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        assert "lora_" in n and p.grad is not None, n
        trainable.append(n)
        out[f"grad_slice::{n}"], out[f"grad_tail::{n}"] = sl(p.grad), p.grad[-3:, -6:].numpy().copy()
        out[f"grad_grid::{n}"] = H.grad_grid(p.grad).numpy().copy()
        out[f"grad_norm::{n}"], out[f"grad_stats::{n}"] = np.array([p.grad.double().norm().item()]), stats(p.grad)
    assert len(trainable) == 2 * len(H.ALL) * H.DEPTH
    out["trainable_names"] = np.array(sorted(trainable))
    path = os.path.join(GOLD, "lora_sites.npz")
    np.savez_compressed(path, **out)
    print("sensitivity [site, tap]:", sens.round(3).tolist())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
