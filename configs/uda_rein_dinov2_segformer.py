# DACS self-training (UDA, GTA -> Cityscapes) around DINOv2-L + Rein + SegformerHead at 512 x 512
# (reference: configs/uda/uda_rein_dinov2_Segformer_512x512.py -> configs/uda/datasets/uda_gta_to_cityscapes_512x512.py,
# configs/_base_/models/rein_dinov2_segformer.py).  blur / colour jitter are switched off: see presets.uda_rein_dinov2_segformer.
from vfmseg_amd import presets

crop_size = (512, 512)
num_classes = 19
model = presets.uda_rein_dinov2_segformer()
_o = presets.optim_cfg()
optim_wrapper = _o["optim_wrapper"]
param_scheduler = _o["param_scheduler"]

# ---- dataset part (configs/_base_/datasets/gta_512x512.py, cityscapes_512x512.py).  The GTA pipeline takes the fixed 1280 x 720 resize the
# reference keeps as a comment: its RandomChoiceResize is not in the input pipeline of this project.
_gta_train_pipeline = [
    dict(type="LoadImageFromFile"),
    dict(type="LoadAnnotations"),
    dict(type="Resize", scale=(1280, 720)),
    dict(type="RandomCrop", crop_size=crop_size, cat_max_ratio=0.75),
    dict(type="RandomFlip", prob=0.5),
    dict(type="PhotoMetricDistortion"),
    dict(type="PackSegInputs"),
]
_cityscapes_train_pipeline = [
    dict(type="LoadImageFromFile"),
    dict(type="LoadAnnotations"),
    dict(type="Resize", scale=(1024, 512)),
    dict(type="RandomCrop", crop_size=crop_size, cat_max_ratio=0.75),
    dict(type="RandomFlip", prob=0.5),
    dict(type="PhotoMetricDistortion"),
    dict(type="PackSegInputs"),
]
train_gta = dict(type="CityscapesDataset", data_root="data/gta/", data_prefix=dict(img_path="images", seg_map_path="labels"),
                 img_suffix=".png", seg_map_suffix="_labelTrainIds.png", pipeline=_gta_train_pipeline)
train_cityscapes = dict(type="CityscapesDataset", data_root="data/cityscapes/",
                        data_prefix=dict(img_path="leftImg8bit/train", seg_map_path="gtFine/train"), pipeline=_cityscapes_train_pipeline)
uda_dataset_train = dict(type="UDADataset", source=train_gta, target=train_cityscapes,
                         rare_class_sampling=dict(class_temp=0.01, min_crop_ratio=0.5, min_pixels=3000))
train_dataloader = dict(batch_size=2, num_workers=4, persistent_workers=True, pin_memory=True,
                        sampler=dict(type="InfiniteSampler", shuffle=True), dataset=uda_dataset_train)

train_cfg = dict(type="IterBasedTrainLoop", max_iters=40000, val_interval=1000)
default_hooks = dict(logger=dict(type="LoggerHook", interval=50), checkpoint=dict(type="CheckpointHook", by_epoch=False, interval=4000, max_keep_ckpts=3))
randomness = dict(seed=0)
env_cfg = dict(dist_cfg=dict(backend="nccl"))
