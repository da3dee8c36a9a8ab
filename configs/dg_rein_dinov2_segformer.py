# DINOv2-L + Rein (LoRAReins, 100 tokens of rank 16) + SegformerHead, sliding-window test (512 / 341)
# (reference: configs/dg/gta2citys/dg_rein_dinov2_Segformer_512x512_bs1x4.py -> configs/_base_/models/rein_dinov2_segformer.py).
from vfmseg_amd import presets

crop_size = (512, 512)
num_classes = 19
model = presets.rein_dinov2_segformer()
_o = presets.optim_cfg()
optim_wrapper = _o["optim_wrapper"]
param_scheduler = _o["param_scheduler"]
randomness = dict(seed=0)
env_cfg = dict(dist_cfg=dict(backend="nccl"))
