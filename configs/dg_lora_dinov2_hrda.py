# DINOv2-L + LoRA + HRDAHead (LinearHead + scale-attention head): the HRDA multi-resolution baseline, 1024^2 training images
# (reference: configs/dg/gta2citys/dg_lora_dinov2_hrda_1024x1024.py -> configs/_base_/models/lora_dinov2_hrda.py).
from vfmseg_amd import presets

crop_size = (1024, 1024)
num_classes = 19
model = presets.dinov2_hrda()
_o = presets.optim_cfg()
optim_wrapper = _o["optim_wrapper"]
param_scheduler = _o["param_scheduler"]
randomness = dict(seed=0)
env_cfg = dict(dist_cfg=dict(backend="nccl"))
