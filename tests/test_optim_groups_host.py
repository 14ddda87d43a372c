"""Host side of the grouped fused AdamW (no device needed): the engine's parameter groups, the folding of (group, step) pairs
into the kernel's classes, the two config keys, and torch.optim.AdamW's checkpoint layout."""
import os
import types

import pytest
import torch


@pytest.fixture(scope="module")
def detector():
    from model import MonoConDetector
    return MonoConDetector(34, pretrained_backbone=False)


def _solver(detector, **optim):
    from engine.monocon_engine import MonoconEngine
    from utils.engine_utils import get_default_cfg
    cfg = get_default_cfg()
    cfg.set_new_allowed(True)
    for k, v in optim.items():
        if k == "NORM_TYPE":
            cfg.SOLVER.CLIP_GRAD.NORM_TYPE = v
        else:
            cfg.SOLVER.OPTIM[k] = v
    stub = types.SimpleNamespace(model=detector, train_loader=[0] * 10, cfg=cfg)
    return cfg, MonoconEngine.build_solver(stub)


def test_build_solver_default_is_the_single_reference_group(detector):
    cfg, (opt, sch) = _solver(detector)
    assert opt.__class__.__name__ == "AdamW" and len(opt.param_groups) == 1
    g = opt.param_groups[0]
    assert [id(p) for p in g["params"]] == [id(p) for p in detector.parameters()]
    assert g["weight_decay"] == cfg.SOLVER.OPTIM.WEIGHT_DECAY == 1e-5 and g["initial_lr"] == cfg.SOLVER.OPTIM.LR == 2.25e-4
    assert g["betas"][1] == 0.99 and g["amsgrad"] is False and g["maximize"] is False
    assert opt.max_grad_norm == 35.0 and opt.norm_type == 2.0 and sch.total_steps == 10 * cfg.SOLVER.OPTIM.NUM_EPOCHS


def test_build_solver_groups(detector):
    """every parameter lands in exactly one group, backbone.* at LR * BACKBONE_LR_MULT, 1-D parameters in the zero-decay twin of
    their group, group 0 the base group; NORM_TYPE reaches the optimizer"""
    cfg, (opt, sch) = _solver(detector, BACKBONE_LR_MULT=0.1, NO_DECAY_NORM_BIAS=True, NORM_TYPE=float("inf"))
    lr, wd = cfg.SOLVER.OPTIM.LR, cfg.SOLVER.OPTIM.WEIGHT_DECAY
    assert opt.norm_type == float("inf")
    assert [(g["initial_lr"], g["weight_decay"]) for g in opt.param_groups] == [(lr, wd), (lr * 0.1, wd), (lr, 0.0), (lr * 0.1, 0.0)]
    assert sch.base_lrs == [lr, lr * 0.1, lr, lr * 0.1]
    where = {}
    for gi, g in enumerate(opt.param_groups):
        for p in g["params"]:
            assert id(p) not in where
            where[id(p)] = gi
    named = list(detector.named_parameters())
    assert len(where) == len(named) and all(len(g["params"]) > 0 for g in opt.param_groups)
    for name, p in named:
        assert where[id(p)] == (1 if name.startswith("backbone.") else 0) + (2 if p.dim() <= 1 else 0), name
    # each option alone
    _, (opt, _) = _solver(detector, BACKBONE_LR_MULT=0.0)
    assert [g["lr"] == 0.0 for g in opt.param_groups] == [False, True]
    assert sum(len(g["params"]) for g in opt.param_groups) == len(named)
    _, (opt, _) = _solver(detector, NO_DECAY_NORM_BIAS=True)
    assert [g["weight_decay"] for g in opt.param_groups] == [wd, 0.0]
    assert all(p.dim() <= 1 for p in opt.param_groups[1]["params"]) and all(p.dim() > 1 for p in opt.param_groups[0]["params"])


def test_class_folding():
    from hipmonocon.lib import MonoconHipError, OptimClass
    from solver.fused_adamw import MAX_CLASSES, fold_classes
    base = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False)
    groups = [dict(base), dict(base, lr=2e-3), dict(base), dict(base, amsgrad=True), dict(base, maximize=True)]
    classes, cls = fold_classes(groups, [(0, 3), (1, 3), (0, 3), (0, 2), (2, 3), (2, 2), (3, 3), (4, 3), (1, 3)])
    # groups 0 and 2 are equal: (0, 3) and (2, 3) are one class, and so are (0, 2) and (2, 2); order of first appearance
    assert cls == (0, 1, 0, 2, 0, 2, 3, 4, 1)
    assert classes == [(1e-3, 0.9, 0.99, 1e-8, 1e-2, 3, False, False), (2e-3, 0.9, 0.99, 1e-8, 1e-2, 3, False, False),
                       (1e-3, 0.9, 0.99, 1e-8, 1e-2, 2, False, False), (1e-3, 0.9, 0.99, 1e-8, 1e-2, 3, True, False),
                       (1e-3, 0.9, 0.99, 1e-8, 1e-2, 3, False, True)]
    tab = (OptimClass * len(classes))(*classes)
    assert (tab[3].lr, tab[3].beta2, tab[3].step, tab[3].amsgrad, tab[3].maximize) == (1e-3, 0.99, 3, 1, 0)
    assert MAX_CLASSES == 16
    many = [dict(base, lr=1e-3 * (k + 1)) for k in range(17)]
    classes, cls = fold_classes(many, [(k, 1) for k in range(16)])
    assert cls == tuple(range(16))
    with pytest.raises(MonoconHipError, match="more than 16"):
        fold_classes(many, [(k, 1) for k in range(17)])
    with pytest.raises(MonoconHipError, match="more than 16"):           # one group, 17 different step counts
        fold_classes([base], [(0, s + 1) for s in range(17)])


REFERENCE_STYLE_YAML = """
DATA:
  BATCH_SIZE: 8
  ROOT: /data/kitti
  FILTER: {MAX_DEPTH: 65, MAX_OCCLUSION: 2, MAX_TRUNCATION: 0.5, MIN_DEPTH: 2, MIN_HEIGHT: 25}
MODEL:
  BACKBONE: {IMAGENET_PRETRAINED: true, NUM_LAYERS: 34}
  HEAD: {MAX_OBJS: 30, NUM_CLASSES: 3}
SOLVER:
  CLIP_GRAD: {ENABLE: true, MAX_NORM: 35, NORM_TYPE: 2.0}
  OPTIM: {LR: 0.000225, NUM_EPOCHS: 200, WEIGHT_DECAY: 1.0e-05}
  SCHEDULER: {ENABLE: true}
PERIOD: {EVAL_PERIOD: 10, LOG_PERIOD: 50}
"""


def test_config_defaults_merge_a_reference_style_yaml(tmp_path):
    from utils.engine_utils import get_default_cfg, load_cfg
    c = get_default_cfg()
    assert c.SOLVER.OPTIM.BACKBONE_LR_MULT == 1.0 and c.SOLVER.OPTIM.NO_DECAY_NORM_BIAS is False
    path = os.path.join(tmp_path, "ref.yaml")
    open(path, "w").write(REFERENCE_STYLE_YAML)
    strict = get_default_cfg()
    strict.merge_from_file(path)            # no new keys allowed: the file's keys all exist in the tree
    loaded = load_cfg(path)
    for c in (strict, loaded):
        assert c.SOLVER.OPTIM.LR == 2.25e-4 and c.SOLVER.OPTIM.BACKBONE_LR_MULT == 1.0 and c.SOLVER.OPTIM.NO_DECAY_NORM_BIAS is False
        assert c.SOLVER.CLIP_GRAD.NORM_TYPE == 2.0 and c.DATA.ROOT == "/data/kitti"
    path2 = os.path.join(tmp_path, "groups.yaml")
    open(path2, "w").write("SOLVER:\n  OPTIM: {BACKBONE_LR_MULT: 0.0, NO_DECAY_NORM_BIAS: true}\n  CLIP_GRAD: {NORM_TYPE: .inf}\n")
    c = get_default_cfg()
    c.merge_from_file(path2)
    assert c.SOLVER.OPTIM.BACKBONE_LR_MULT == 0.0 and c.SOLVER.OPTIM.NO_DECAY_NORM_BIAS is True
    assert c.SOLVER.CLIP_GRAD.NORM_TYPE == float("inf") and c.SOLVER.OPTIM.LR == 2.25e-4


def test_state_dict_layout_is_torch_optim_adamw_s():
    """key for key: top level, every group, every parameter's state -- including max_exp_avg_sq of the amsgrad group only"""
    from solver import AdamW

    def make(cls):
        torch.manual_seed(0)
        ps = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2))]
        return ps, cls([dict(params=ps[:2], amsgrad=True), dict(params=ps[2:], lr=1e-2, weight_decay=0.0)], lr=1e-3, betas=(0.9, 0.99))

    pt, ot = make(torch.optim.AdamW)
    for p in pt[:2] + pt[2:]:
        p.grad = torch.ones_like(p)
    ot.step()
    ref = ot.state_dict()
    pf, of = make(AdamW)
    fresh = of.state_dict()
    assert set(fresh) == set(ref) and fresh["state"] == {}
    assert [set(g) for g in fresh["param_groups"]] == [set(g) for g in ref["param_groups"]]
    assert [g["params"] for g in fresh["param_groups"]] == [g["params"] for g in ref["param_groups"]]
    for ga, gb in zip(fresh["param_groups"], ref["param_groups"]):
        assert all(ga[k] == gb[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"))
    # the state the fused step creates lazily, per parameter
    for p, g in ((pf[0], of.param_groups[0]), (pf[2], of.param_groups[1])):
        of._init_state(p, g["amsgrad"])
    lazy = of.state_dict()["state"]
    assert set(lazy[0]) == set(ref["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    assert set(lazy[2]) == set(ref["state"][2]) == {"step", "exp_avg", "exp_avg_sq"}
    assert lazy[0]["step"].dtype == ref["state"][0]["step"].dtype and lazy[0]["step"].shape == ref["state"][0]["step"].shape
    # torch's checkpoint in, the same checkpoint out
    of.load_state_dict(ref)
    back = of.state_dict()
    assert set(back["state"]) == set(ref["state"])
    for k, st in ref["state"].items():
        assert set(back["state"][k]) == set(st)
        assert all(torch.equal(back["state"][k][n], st[n]) for n in st)
        assert all(back["state"][k][n] is not st[n] for n in st)       # private copies: step() updates them in place
    assert [set(g) for g in back["param_groups"]] == [set(g) for g in ref["param_groups"]]
    ot2 = make(torch.optim.AdamW)[1]
    ot2.load_state_dict(back)                                            # and torch takes it back
    assert float(ot2.state[ot2.param_groups[0]["params"][0]]["step"]) == 1.0
