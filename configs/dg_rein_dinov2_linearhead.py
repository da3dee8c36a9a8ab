# DINOv2-L + Rein (LoRAReins, 100 tokens of rank 16) + LinearHead, sliding-window test
# (reference: configs/dg/gta2citys/dg_rein_dinov2_linearhead.py -> configs/_base_/models/rein_dinov2_linear.py).
from vfmseg_amd import presets

crop_size = (512, 512)
num_classes = 19
model = presets.rein_dinov2_linear()
_o = presets.optim_cfg()
optim_wrapper = _o["optim_wrapper"]
param_scheduler = _o["param_scheduler"]
randomness = dict(seed=0)
env_cfg = dict(dist_cfg=dict(backend="nccl"))
