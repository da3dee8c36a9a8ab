# DINOv2-L + LoRA (r=32) on every linear layer of a block (qkv, attn.proj, fc1, fc2) + LinearHead: the "all linear layers" recipe of the
# LoRA ablation.  Otherwise the linear-head LoRA model (presets.dinov2_linear: one 512^2 pass per sample, whole-image test).
from vfmseg_amd import presets

crop_size = (512, 512)
num_classes = 19
model = presets.dinov2_linear()
model["backbone"]["Lora_config"] = presets.lora_cfg(target_modules=presets.ALL_LINEAR)
_o = presets.optim_cfg()
optim_wrapper = _o["optim_wrapper"]
param_scheduler = _o["param_scheduler"]
randomness = dict(seed=0)
env_cfg = dict(dist_cfg=dict(backend="nccl"))
