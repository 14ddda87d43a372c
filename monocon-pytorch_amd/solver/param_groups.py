"""Parameter groups of the detector for the fused AdamW (SOLVER.OPTIM.BACKBONE_LR_MULT / NO_DECAY_NORM_BIAS).

Group 0 is always the base group (``lr``, ``weight_decay`` as configured): ``BaseEngine.current_lr`` and the log line
read it.  Every ``backbone.*`` parameter goes to a group at ``lr * backbone_lr_mult``; with ``no_decay_norm_bias`` every
1-D parameter (norm weights and biases, conv biases) goes to a zero-decay twin of its group.  With both options at
their defaults the result is one group holding ``named_parameters()`` in order -- the reference's single group.
A multiplier of 0 freezes the backbone THROUGH THE OPTIMIZER: its weights stay bit-unchanged, its moments, its
gradients and its BatchNorm running statistics are still computed.  Pure host code.
"""


def build_param_groups(named_parameters, lr, weight_decay, backbone_lr_mult=1.0, no_decay_norm_bias=False,
                       backbone_prefix="backbone."):
    named = [(n, p) for n, p in named_parameters]
    split_backbone = float(backbone_lr_mult) != 1.0
    table = {}                          # (is_backbone, is_no_decay) -> group

    def group_of(name, p):
        bb = split_backbone and name.startswith(backbone_prefix)
        nd = bool(no_decay_norm_bias) and p.dim() <= 1
        g = table.get((bb, nd))
        if g is None:
            g = table[(bb, nd)] = {"params": [], "lr": lr * backbone_lr_mult if bb else lr,
                                   "weight_decay": 0.0 if nd else weight_decay}
        return g

    base = table[(False, False)] = {"params": [], "lr": lr, "weight_decay": weight_decay}
    for name, p in named:
        group_of(name, p)["params"].append(p)
    order = [(False, False), (True, False), (False, True), (True, True)]
    groups = [table[k] for k in order if k in table and (table[k]["params"] or table[k] is base)]
    return groups
