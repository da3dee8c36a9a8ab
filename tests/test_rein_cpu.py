"""Rein adapters, CPU side: the reference's own Rein config builds through the registry (where the reference tree exists), the optimiser /
data-parallel grouping of the `reins` parameters, and the float64 restatement of the adapter step (tests/rein_helpers.py) against the
reference-made fixture - which is what lets the GPU tests, on a box without the reference, compare against that restatement."""
import hashlib
import os

import numpy as np
import pytest
import torch

import vfmseg_amd  # noqa: F401
from tests.helpers import model_shapes, rel_err, sl, stats
from tests.rein_helpers import rein_params, rein_step_f64, step_inputs
from vfmseg_amd import presets
from vfmseg_amd.config import Config
from vfmseg_amd.optim import param_options, production_order
from vfmseg_amd.parallel import make_buckets
from vfmseg_amd.registry import MODELS

REF = "/root/reference/configs/dg/gta2citys"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")


def _shrunk_reference_model():
    cfg = Config.fromfile(os.path.join(REF, "dg_rein_dinov2_linearhead.py"))
    m = cfg.model
    m["backbone"].update(depth=2, out_indices=[0, 1, 1, 1])      # build time only, as test_reference_configs_cpu.py cuts the depth
    m["backbone"]["reins_config"]["num_layers"] = 2
    m["backbone"]["init_cfg"]["checkpoint"] = None                  # no weights offline
    return cfg, MODELS.build(m)


@needs_ref
def test_reference_rein_config_builds_unchanged(golden_dir):
    cfg, model = _shrunk_reference_model()
    assert type(model).__name__ == "EncoderDecoder" and type(model.backbone).__name__ == "ReinsDinoVisionTransformer"
    keys = set(model.state_dict())
    assert keys and all(k.startswith("backbone.reins.") or k.startswith("decode_head.") for k in keys), sorted(keys)[:5]
    for k in ("scale", "learnable_tokens_a", "learnable_tokens_b", "mlp_token2feat.weight", "mlp_delta_f.bias", "transform.weight", "merge.bias"):
        assert "backbone.reins." + k in keys, k
    model.train()
    G = np.load(os.path.join(golden_dir, "rein.npz"))
    live = {"backbone." + str(n) for n in G["full_live_params"]}
    got = {n for n, p in model.named_parameters() if p.requires_grad and n.startswith("backbone.")}
    assert got == live, got ^ live
    frozen = {"backbone." + str(n) for n in G["full_no_grad_params"]}     # transform / merge never enter the graph
    assert frozen and all(not dict(model.named_parameters())[n].requires_grad for n in frozen)
    assert not model.backbone.blocks[0].training and model.backbone.reins.training and model.decode_head.training
    ow = cfg.optim_wrapper
    opts = param_options(model, ow["optimizer"]["lr"], ow["optimizer"]["weight_decay"], ow.get("paramwise_cfg"))
    for n, (lr_mult, wd) in opts.items():
        if "learnable_tokens" in n or n.endswith("reins.scale"):
            assert (lr_mult, wd) == (1.0, 0.0), (n, lr_mult, wd)
        elif n.startswith("backbone.reins."):
            assert wd == ow["optimizer"]["weight_decay"], (n, wd)
    assert sum("learnable_tokens" in n for n in opts) == 2 and "backbone.reins.scale" in opts
    model.eval()
    assert not model.backbone.reins.training and not model.backbone.adapter_training()


@needs_ref
def test_reference_rein_config_equals_preset():
    from tests.test_reference_configs_cpu import ALLOWED, _diff, _plain
    cfg = Config.fromfile(os.path.join(REF, "dg_rein_dinov2_linearhead.py"))
    bad = [d for d in _diff(_plain(cfg.model), _plain(presets.rein_dinov2_linear())) if not any(a in d[0] for a in ALLOWED)]
    assert not bad, bad[:8]
    ours = Config.fromfile(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "dg_rein_dinov2_linearhead.py"))
    assert _plain(ours.model) == _plain(presets.rein_dinov2_linear())
    assert _plain(ours.optim_wrapper) == _plain(cfg.optim_wrapper)


@pytest.mark.parametrize("kw", [dict(use_softmax=False), dict(zero_mlp_delta_f=True), dict(link_token_to_query=True)])
def test_unsupported_rein_options_say_why(kw):
    cfg = dict(presets.reins_cfg(depth=2, embed_dim=64), **kw)
    with pytest.raises(NotImplementedError):
        MODELS.build(cfg)


def test_plain_reins_registered_with_reference_keys():
    r = MODELS.build(dict(type="Reins", num_layers=2, embed_dims=64, patch_size=16, token_length=10, link_token_to_query=False))
    assert set(r.state_dict()) == {"learnable_tokens", "scale", "mlp_token2feat.weight", "mlp_token2feat.bias", "mlp_delta_f.weight",
                                   "mlp_delta_f.bias", "transform.weight", "transform.bias", "merge.weight", "merge.bias"}
    assert r.scale.dim() == 0 and abs(float(r.scale.detach()) - 0.001) < 1e-9
    val = (6.0 / (3 * 16 * 16 + 64)) ** 0.5
    assert float(r.learnable_tokens.detach().abs().max()) <= val


# ---------------------------------------------------------------- the frozen base arrives through init_cfg (rein_dinov2_linear.py:38-41)
def _small_cfg(checkpoint):
    cfg = presets.rein_dinov2_linear(depth=2, embed_dim=64, num_heads=2, checkpoint=checkpoint)
    cfg["backbone"].update(img_size=64, out_indices=[0, 1, 1, 1])
    cfg["decode_head"]["norm_cfg"] = dict(type="GN", num_groups=8)
    return cfg


def test_init_cfg_pretrained_loads_the_frozen_base(tmp_path):
    """A bare DINOv2 state dict on disk, named by the config as the reference names it: the built model's base equals it, state_dict() still
    holds rein + head keys only, training leaves the base frozen; a file whose keys do not match is an error, not an untrained base."""
    donor = MODELS.build(dict({k: v for k, v in _small_cfg(None)["backbone"].items() if k not in ("reins_config", "init_cfg")},
                              type="DinoVisionTransformer"))
    g = torch.Generator().manual_seed(3)
    bare = {k: torch.randn(v.shape, generator=g) for k, v in donor.state_dict().items()}
    path = tmp_path / "dinov2_converted.pth"
    torch.save(bare, path)
    model = MODELS.build(_small_cfg(str(path)))
    assert model.backbone.pretrained == str(path)
    named = dict(model.backbone.named_parameters())
    base = [k for k in named if not k.startswith("reins.")]
    assert set(base) == set(bare) and all(torch.equal(named[k].detach(), bare[k]) for k in base)
    assert all(k.startswith("backbone.reins.") or k.startswith("decode_head.") for k in model.state_dict())
    model.train()
    assert all(not named[k].requires_grad for k in base)
    # without a checkpoint the base keeps its initialisers (and says so)
    assert MODELS.build(_small_cfg(None)).backbone.pretrained is None
    # keys under a wrong prefix: refused
    wrong = tmp_path / "wrong.pth"
    torch.save({"backbone." + k: v for k, v in bare.items()}, wrong)
    with pytest.raises(RuntimeError, match="base parameters not found"):
        MODELS.build(_small_cfg(str(wrong)))
    with pytest.raises(NotImplementedError):
        MODELS.build(dict(_small_cfg(None)["backbone"], init_cfg=dict(type="Kaiming", checkpoint=str(path))))


def test_runner_keeps_a_pretrained_base(tmp_path, monkeypatch):
    """Runner.from_cfg's synthetic initialisation (no checkpoints offline) must not overwrite a base that init_cfg loaded."""
    from vfmseg_amd import runner as Rn
    src = MODELS.build(_small_cfg(None)).backbone
    bare = {k: v.detach().clone() + 0.5 for k, v in src.named_parameters() if not k.startswith("reins.")}
    path = tmp_path / "base.pth"
    torch.save(bare, path)
    built = {}

    class _Stop(Exception):
        pass

    def fake_cuda(self):
        built["m"] = self
        raise _Stop()
    monkeypatch.setattr(torch.nn.Module, "cuda", fake_cuda)
    monkeypatch.setattr(Rn.parallel, "init_from_env", lambda: (0, 1, 0))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for ck in (str(path), None):
        with pytest.raises(_Stop):
            Rn.Runner.from_cfg(dict(model=_small_cfg(ck)))
        named = dict(built["m"].backbone.named_parameters())
        same = all(torch.equal(named[k].detach(), bare[k]) for k in bare)
        assert same == (ck is not None)


# ---------------------------------------------------------------- gradient-production order / DP buckets
def _trainable_names(depth, rein=False):
    out = [k for k in model_shapes(depth) if not (k.startswith("backbone.") and "lora_" not in k) and "running_" not in k and "num_batches" not in k]
    if rein:
        out = [k for k in out if k.startswith("decode_head.")]
        out += ["backbone.reins." + k for k in ("scale", "learnable_tokens_a", "learnable_tokens_b", "mlp_token2feat.weight",
                                                "mlp_token2feat.bias", "mlp_delta_f.weight", "mlp_delta_f.bias")]
    return out


def _offsets(depth, order, extra=None):
    shp = dict(model_shapes(depth))
    shp.update(extra or {})
    offs = [0]
    for k in order:
        s = shp[k]
        n = 1 if (len(s) == 2 and isinstance(s[1], torch.dtype)) else int(np.prod(s))
        offs.append((offs[-1] + n + 15) // 16 * 16)
    return offs


# production order (sha256 of the joined names) and buckets of the LoRA ms_masked model as the commit before the Rein group computed them
PARENT = {24: ("a46cd607757efee314d6758b5a91e98c056d844eaba588ab29eb1b557f4eb07e",
               [("aux_decoder", 0, 6644832), ("decode_head", 6644832, 13469312), ("lora0", 13469312, 15042176), ("lora1", 15042176, 16615040)]),
          4: ("e18ed1e44844eb1995c8e98fcafebf2aa0d88c2b69d1617ca47d2a123c36a23e",
              [("aux_decoder", 0, 6644832), ("decode_head", 6644832, 13469312), ("lora0", 13469312, 13731456), ("lora1", 13731456, 13993600)])}


@pytest.mark.parametrize("depth", [24, 4])
def test_lora_model_order_and_buckets_unchanged(depth):
    order = production_order(_trainable_names(depth))
    assert hashlib.sha256("\n".join(order).encode()).hexdigest() == PARENT[depth][0]
    assert make_buckets(order, _offsets(depth, order)) == PARENT[depth][1]


def test_rein_group_is_last_and_not_a_head_bucket():
    names = _trainable_names(4, rein=True)
    order = production_order(list(reversed(names)))
    nr = sum(n.startswith("backbone.reins.") for n in names)
    assert nr == 7 and all(n.startswith("backbone.reins.") for n in order[-nr:]) and all(n.startswith("decode_head.") for n in order[:-nr])
    extra = {"backbone.reins.scale": (), "backbone.reins.learnable_tokens_a": (4, 100, 16), "backbone.reins.learnable_tokens_b": (4, 16, 1024),
             "backbone.reins.mlp_token2feat.weight": (1024, 1024), "backbone.reins.mlp_token2feat.bias": (1024,),
             "backbone.reins.mlp_delta_f.weight": (1024, 1024), "backbone.reins.mlp_delta_f.bias": (1024,)}
    offs = _offsets(4, order, extra)
    buckets = make_buckets(order, offs)
    assert [b[0] for b in buckets] == ["decode_head", "reins"]
    assert buckets[1][1] == offs[len(order) - nr] and buckets[1][2] == offs[-1] and buckets[0][2] == buckets[1][1]
    # what parallel.attach launches when the backbone backward STARTS must leave the shared Rein gradients alone
    head_ids = [i for i, b in enumerate(buckets) if not b[0].startswith("lora") and b[0] != "reins"]
    assert head_ids == [0]


def test_grad_sync_wiring_sends_rein_bucket_after_the_backbone(monkeypatch):
    """parallel.attach with a stub process group: heads_done readies the head bucket only, backbone_done the `reins` bucket."""
    import types
    from vfmseg_amd import backbones, parallel
    names = production_order(_trainable_names(4, rein=True))
    sent = []

    class _GS:
        def __init__(self, gflat, buckets, group=None):
            self.buckets = buckets

        def ready(self, i):
            sent.append(self.buckets[i][0])

    monkeypatch.setattr(parallel, "GradSync", _GS)
    monkeypatch.setattr(parallel, "broadcast_params", lambda m: None)
    monkeypatch.setattr(parallel.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(parallel.dist, "get_world_size", lambda g=None: 2)
    offs = list(range(0, 16 * (len(names) + 1), 16))
    ow = types.SimpleNamespace(optimizer=types.SimpleNamespace(names=names, offsets=offs, gflat=None), grad_sync=None)
    saved = dict(backbones.BACKWARD_EVENTS)
    try:
        parallel.attach(types.SimpleNamespace(), ow)
        backbones.BACKWARD_EVENTS["heads_done"]()
        assert sent == ["decode_head"]
        backbones.BACKWARD_EVENTS["backbone_done"]()
        assert sent == ["decode_head", "reins"]
    finally:
        backbones.BACKWARD_EVENTS.update(saved)


# ---------------------------------------------------------------- the float64 restatement is pinned to the reference
@pytest.mark.parametrize("lora", [True, False])
def test_f64_restatement_equals_reference_fixture(golden_dir, lora):
    G = np.load(os.path.join(golden_dir, "rein.npz"))
    tag = "lora" if lora else "plain"
    x, g = step_inputs()
    xo, dx, grads, _ = rein_step_f64(x, g, rein_params(depth=4, lora=lora), 3)
    assert rel_err(sl(xo), G[f"step_{tag}_xo_slice"]) < 1e-6 and rel_err(sl(dx), G[f"step_{tag}_dx_slice"]) < 1e-6
    np.testing.assert_allclose(stats(xo), G[f"step_{tag}_xo_stats"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(stats(dx), G[f"step_{tag}_dx_stats"], rtol=1e-6, atol=1e-9)
    seen = 0
    for key in G.files:
        if key.startswith(f"step_{tag}_grad_slice::"):
            n = key.split("::", 1)[1]
            gr = grads[n][3] if n.startswith("learnable_tokens") else grads[n]
            gr = gr.reshape(1, -1) if gr.dim() < 2 else gr
            assert rel_err(sl(gr), G[key]) < 1e-6, n
            np.testing.assert_allclose(grads[n].norm().item(), G[f"step_{tag}_grad_norm::{n}"][0], rtol=1e-6)
            seen += 1
    assert seen == len(grads) == (7 if lora else 6)
    assert sorted(str(n) for n in G[f"step_{tag}_no_grad"]) == ["merge.bias", "merge.weight", "transform.bias", "transform.weight"]
    ratio, top = G[f"step_{tag}_token_term_ratio_top_prob"]
    assert ratio >= 0.3 and 0.1 <= top <= 0.9
    assert (G["full_tap_sensitivity"] >= 0.3).all()
