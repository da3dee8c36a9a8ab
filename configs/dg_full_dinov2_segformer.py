# Full fine-tuning: DINOv2-L with every backbone weight trained + SegformerHead, sliding-window test (512 / 341) - the "Full" row of the
# PEFT comparisons (mmseg's plain EncoderDecoder over the bare DinoVisionTransformer of configs/_base_/models/dinov2_SegFormer_frozen.py).
# The pretrained backbone steps at a tenth of the head's learning rate; LayerNorms are not decayed.
from vfmseg_amd import presets

crop_size = (512, 512)
num_classes = 19
model = presets.full_dinov2_segformer()
_o = presets.optim_cfg(backbone_lr_mult=0.1)
optim_wrapper = _o["optim_wrapper"]
param_scheduler = _o["param_scheduler"]
randomness = dict(seed=0)
env_cfg = dict(dist_cfg=dict(backend="nccl"))
