# DINOv2-L + LoRA (r=32 on qkv) + SegformerHead, sliding-window test (512 / 341)
# (reference: configs/dg/gta2citys/dg_lora_dinov2_SegFormer.py -> configs/_base_/models/lora_dinov2_SegFormer.py).
from vfmseg_amd import presets

crop_size = (512, 512)
num_classes = 19
model = presets.dinov2_segformer()
_o = presets.optim_cfg()
optim_wrapper = _o["optim_wrapper"]
param_scheduler = _o["param_scheduler"]
randomness = dict(seed=0)
env_cfg = dict(dist_cfg=dict(backend="nccl"))
