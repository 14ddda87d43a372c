"""Default configuration tree.  Keys and default values are those of the reference's yacs tree
(config/monocon_configs.py:4-64) so its YAML files merge unchanged; kept here as one nested table."""
from config.cfgnode import CfgNode as CN

_DEFAULTS = {
    "VERSION": "v1.0.3",
    "DESCRIPTION": "MonoCon Default Configuration",
    "OUTPUT_DIR": "",
    "SEED": -1,
    "GPU_ID": 0,
    "USE_BENCHMARK": True,
    "DATA": {
        # 'synthetic' selects the built-in KITTI-shaped synthetic dataset; anything else is a KITTI root directory
        "ROOT": r"/home/user/SSD/KITTI",
        "BATCH_SIZE": 8,
        "NUM_WORKERS": 4,
        "TRAIN_SPLIT": "train",
        "TEST_SPLIT": "val",
        # [H, W]: run the network at this resolution (Resize3D first in both transform lists, resampled on the device with the
        # frames' other image work); [] = the frames keep their size
        "RESIZE_HW": [],
        "FILTER": {"MIN_HEIGHT": 25, "MIN_DEPTH": 2, "MAX_DEPTH": 65, "MAX_TRUNCATION": 0.5, "MAX_OCCLUSION": 2},
    },
    "MODEL": {
        "BACKBONE": {"NUM_LAYERS": 34, "IMAGENET_PRETRAINED": True},
        "HEAD": {"NUM_CLASSES": 3, "MAX_OBJS": 30},
    },
    "SOLVER": {
        # BACKBONE_LR_MULT / NO_DECAY_NORM_BIAS (not in the reference's tree; their defaults are its single parameter group):
        # learning rate of the backbone.* parameters relative to LR (0.0 holds them still), and no weight decay on 1-D
        # parameters (norm weights and biases, conv biases) -- solver/param_groups.py
        "OPTIM": {"LR": 2.25e-4, "WEIGHT_DECAY": 1e-5, "NUM_EPOCHS": 200, "BACKBONE_LR_MULT": 1.0, "NO_DECAY_NORM_BIAS": False},
        "SCHEDULER": {"ENABLE": True},
        "CLIP_GRAD": {"ENABLE": True, "NORM_TYPE": 2.0, "MAX_NORM": 35},
        # EMA (not in the reference's tree; off = its loop): an exponential moving average of the weights and BatchNorm
        # statistics, updated inside the fused AdamW step, used by evaluate() and kept in the checkpoints -- solver/model_ema.py
        "EMA": {"ENABLE": False, "DECAY": 0.9998, "WARMUP": True},
        # NONFINITE_GUARD (not in the reference's tree; off = its loop): the fused AdamW step skips itself, on the device, when
        # the gradient norm is NaN or infinite; the loop reports the step one iteration late and gives up after
        # MAX_CONSECUTIVE skipped steps in a row -- solver/fused_adamw.py (skip_nonfinite)
        "NONFINITE_GUARD": {"ENABLE": False, "MAX_CONSECUTIVE": 10},
        # ACCUM_STEPS (not in the reference's tree; 1 = its loop): N > 1 takes one optimizer step per window of N batches, on the
        # mean of their gradients (global batch N x BATCH_SIZE on one device; every batch back-propagates its unscaled loss,
        # BatchNorm statistics stay per batch, an epoch's last len(loader) % N batches step as a window of their own) --
        # solver/grad_accum.py
        "ACCUM_STEPS": 1,
        # LAMB (not in the reference's tree; off = its AdamW step): every tensor's update, weight decay included, is rescaled by
        # its trust ratio |p| / |update| inside the fused step, for batches far larger than the 8 the recipe was tuned at.
        # TRUST_CLIP > 0 caps the ratio; ALWAYS_ADAPT also adapts groups without weight decay (NO_DECAY_NORM_BIAS).  LR is still
        # used exactly as configured -- solver/fused_adamw.py (trust_ratio)
        "LAMB": {"ENABLE": False, "TRUST_CLIP": 0.0, "ALWAYS_ADAPT": False},
    },
    "PERIOD": {"EVAL_PERIOD": 10, "LOG_PERIOD": 50},
}


def _tree(table):
    node = CN()
    for key, value in table.items():
        node[key] = _tree(value) if isinstance(value, dict) else value
    return node


_C = _tree(_DEFAULTS)
