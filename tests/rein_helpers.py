"""Helpers of the Rein tests (no reference tree needed): the synthetic Rein parameters, the bare-DINOv2 + head state dict around them,
the seeded inputs of the one-step fixture, and a float64 restatement of the adapter step written from its formulas
(rein/models/backbones/reins.py:84-116 and its backward under autograd).  tools/gen_rein_golden.py uses the same recipe, so the fixture
(tests/golden/rein.npz, written by the reference's own modules) and the tests see identical parameters."""
import zlib

import torch

from tests.helpers import model_shapes
from vfmseg_amd.synth import synth_state_dict

# The default initialisation would make every comparison blind (scale = 0.001 moves the taps by ~1 % of their range, std-0.02 weights shrink
# the token term far below x).  Each tensor = FACTOR * randn seeded by crc32(key); scale is the constant below.
REIN_FACTORS = {"learnable_tokens_a": 1.0, "learnable_tokens_b": 0.3, "learnable_tokens": 1.2, "mlp_token2feat.weight": 0.2,
                "mlp_delta_f.weight": 0.03, "mlp_token2feat.bias": 0.02, "mlp_delta_f.bias": 0.02, "transform.weight": 0.02,
                "transform.bias": 0.02, "merge.weight": 0.02, "merge.bias": 0.02}
REIN_SCALE = 0.05


def _randn(key, shape):
    g = torch.Generator(device="cpu")
    g.manual_seed(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float32)


def rein_shapes(depth=24, dim=1024, m=100, r=16, lora=True, query=256):
    s = {"scale": (), "mlp_token2feat.weight": (dim, dim), "mlp_token2feat.bias": (dim,), "mlp_delta_f.weight": (dim, dim),
         "mlp_delta_f.bias": (dim,), "transform.weight": (query, dim), "transform.bias": (query,), "merge.weight": (query, 3 * query),
         "merge.bias": (query,)}
    if lora:
        s["learnable_tokens_a"], s["learnable_tokens_b"] = (depth, m, r), (depth, r, dim)
    else:
        s["learnable_tokens"] = (depth, m, dim)
    return s


def rein_params(depth=24, dim=1024, m=100, r=16, lora=True):
    """{name under `reins.`: tensor} of the recipe above."""
    out = {}
    for k, shp in rein_shapes(depth, dim, m, r, lora).items():
        out[k] = torch.tensor(REIN_SCALE) if k == "scale" else REIN_FACTORS[k] * _randn("reins." + k, shp)
    return out


def bare_dinov2_state_dict(depth=24, dim=1024):
    """Synthetic weights of the bare DINOv2 keys, as tests/helpers.full_state_dict builds the frozen base of the LoRA model."""
    bb = "backbone.model.base_model.model."
    bare = {k[len(bb):].replace(".base_layer", ""): v for k, v in model_shapes(depth, dim).items() if k.startswith(bb) and "lora_" not in k}
    return synth_state_dict(bare)


def rein_backbone_state_dict(depth=24, dim=1024, lora=True):
    sd = bare_dinov2_state_dict(depth, dim)
    sd.update({"reins." + k: v for k, v in rein_params(depth, dim, lora=lora).items()})
    return sd


def rein_model_state_dict(depth=4, dim=1024):
    """EncoderDecoder(ReinsDinoVisionTransformer, LinearHead): backbone.* + decode_head.*"""
    sd = {"backbone." + k: v for k, v in rein_backbone_state_dict(depth, dim).items()}
    sd.update(synth_state_dict({k: v for k, v in model_shapes(depth, dim).items() if k.startswith("decode_head.")}))
    return sd


def step_inputs(rows=2048, dim=1024, seed=0):
    """x (std 2) and the incoming gradient of the one-step fixture."""
    g = torch.Generator(device="cpu")
    g.manual_seed(4100 + seed)
    return 2.0 * torch.randn(rows, dim, generator=g), torch.randn(rows, dim, generator=g)


def rein_step_f64(x, g, prm, layer):
    """The adapter step and its backward in float64, from the formulas.  x, g [rows, D]; prm as rein_params() (either token form).
    Returns x', dx and {parameter name: gradient} (token gradients of `layer` only, in the parameter's full shape)."""
    P = {k: v.double() for k, v in prm.items()}
    x, g = x.double(), g.double()
    D = x.shape[1]
    c = D ** -0.5
    lora = "learnable_tokens_a" in P
    T = P["learnable_tokens_a"][layer] @ P["learnable_tokens_b"][layer] if lora else P["learnable_tokens"][layer]
    Wt, bt, Wd, bd, s = P["mlp_token2feat.weight"], P["mlp_token2feat.bias"], P["mlp_delta_f.weight"], P["mlp_delta_f.bias"], P["scale"]
    Pm = torch.softmax(c * x @ T.t(), dim=-1)
    V = T[1:] @ Wt.t() + bt
    u = Pm[:, 1:] @ V + x
    y = u @ Wd.t() + bd
    xo = x + s * y
    # backward
    dy = s * g
    grads = {"mlp_delta_f.weight": dy.t() @ u, "mlp_delta_f.bias": dy.sum(0), "scale": (g * y).sum()}
    du = dy @ Wd
    dP = torch.zeros_like(Pm)
    dP[:, 1:] = du @ V.t()
    dS = c * Pm * (dP - (Pm * dP).sum(-1, keepdim=True))
    dx = g + du + dS @ T
    dV = Pm[:, 1:].t() @ du
    dT = dS.t() @ x
    dT[1:] += dV @ Wt
    grads["mlp_token2feat.weight"], grads["mlp_token2feat.bias"] = dV.t() @ T[1:], dV.sum(0)
    if lora:
        ga, gb = torch.zeros_like(P["learnable_tokens_a"]), torch.zeros_like(P["learnable_tokens_b"])
        ga[layer], gb[layer] = dT @ P["learnable_tokens_b"][layer].t(), P["learnable_tokens_a"][layer].t() @ dT
        grads["learnable_tokens_a"], grads["learnable_tokens_b"] = ga, gb
    else:
        gt = torch.zeros_like(P["learnable_tokens"])
        gt[layer] = dT
        grads["learnable_tokens"] = gt
    return xo, dx, grads, dict(P=Pm, u=u, V=V, T=T, du=du, dS=dS)
