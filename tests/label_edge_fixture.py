"""Readers of tests/golden/targets_edge.npz (make_targets_edge_golden.py), shared by the CPU test of the oracle
(test_oracle_label_edges.py) and the GPU test of the kernels (test_hip_label_edges.py).  Not a test module."""
import numpy as np
import torch

from conftest import load_golden
from hipmonocon import synth

GROUPS = ("edge", "dead", "invisible", "kitti")
HEAT = ("center_heatmap_pred", "kpt_heatmap_pred")
LABEL_KEYS = ("gt_bboxes", "gt_labels", "gt_bboxes_3d", "gt_labels_3d", "centers2d", "depths", "gt_kpts_2d",
              "gt_kpts_valid_mask", "mask")
TARGET_KEYS = ("center_heatmap_target", "wh_target", "offset_target", "dim_target", "alpha_cls_target", "alpha_offset_target",
               "depth_target", "center2kpt_offset_target", "kpt_heatmap_target", "kpt_heatmap_offset_target", "indices",
               "indices_kpt", "mask_target", "mask_center2kpt_offset", "mask_kpt_heatmap_offset")
LO, HI = np.float32(1e-4), np.float32(1 - 1e-4)          # what clamp(sigmoid(x), 1e-4, 1 - 1e-4) returns in fp32


class Group:
    """one group of the fixture: labels, the reference's targets, the prediction maps, recorded losses / gradients"""

    def __init__(self, name):
        g = load_golden("targets_edge.npz")
        assert name in [str(s) for s in g["groups"]]
        self.name, self.g = name, g
        self.B, self.H, self.W = (int(v) for v in g[name + ".shape"])
        self.fh, self.fw = self.H // 4, self.W // 4

    def __getitem__(self, key):
        return self.g["%s.%s" % (self.name, key)]

    def labels(self):
        return {k: torch.from_numpy(self["in." + k].copy()) for k in LABEL_KEYS}

    def targets(self):
        """the reference's 15 target tensors, shapes and dtypes as TargetGenerator returns them"""
        return {k: torch.from_numpy(self[k].copy()) for k in TARGET_KEYS}

    def exp_table(self):
        return [(self["exp.arg%d" % i], self["exp.out%d" % i]) for i in range(int(self["exp.n"]))]

    def preds(self):
        """fp32 prediction maps: synth.make_decode_inputs(seed) with the recorded entries put on the two clamp values"""
        d = synth.make_decode_inputs(int(self["pred.seed"]), self.B, self.fh, self.fw)
        for k in HEAT:
            flat = d[k].reshape(-1)
            flat[self["clamp_lo." + k]] = LO
            flat[self["clamp_hi." + k]] = HI
            n = self["n_on_clamp." + k]
            assert (int((flat == LO).sum()), int((flat == HI).sum())) == (int(n[0]), int(n[1])) and n.min() >= 24
        return {k: torch.from_numpy(v) for k, v in d.items()}

    def weights(self):
        return torch.from_numpy(self.g["loss_weights"].copy())


def golden_exp(monkeypatch, table):
    """replace Tensor.exp by the reference host's recorded results (test_targets_exact explains why); returns the set that
    collects the indices of the table entries used"""
    from conftest import rel_err
    host_exp = torch.Tensor.exp
    used = set()

    def exp(x):
        a = x.detach().numpy()
        for i, (arg, out) in enumerate(table):
            if a.dtype == arg.dtype and a.shape == arg.shape and np.array_equal(a.view(np.uint32), arg.view(np.uint32)):
                used.add(i)
                ref = torch.from_numpy(out.copy())
                assert rel_err(host_exp(x), ref) < 1e-6          # (it is an exp table)
                return ref
        raise AssertionError("exp of an argument the reference never took, shape %s" % (tuple(x.shape),))

    monkeypatch.setattr(torch.Tensor, "exp", exp)
    return used


def weighted_total(L, w):
    return sum(w[i].to(torch.as_tensor(v).dtype) * v for i, v in enumerate(L.values()))


def raw_leaves(preds, dtype=torch.float64):
    """(raw, act): pre-activation maps as autograd leaves in `dtype` and the prediction maps rebuilt from them, as
    test_loss_gradients_vs_autograd does: an entry on a clamp value was produced by a logit strictly beyond it."""
    raw = {}
    for k, v in preds.items():
        if k in HEAT:
            x = torch.logit(v.to(dtype))
            x = torch.where(v <= LO, x - 1.0, torch.where(v >= HI, x + 1.0, x))       # compared in fp32, as produced
        elif k == "depth_pred":
            x = torch.cat([torch.logit(1.0 / (v[:, 0:1].to(dtype) + 1.0)), v[:, 1:2].to(dtype)], 1)
        else:
            x = v.to(dtype)
        raw[k] = x.clone().requires_grad_(True)
    act = {}
    for k, v in raw.items():
        if k in HEAT:
            act[k] = torch.clamp(torch.sigmoid(v), 1e-4, 1 - 1e-4)
        elif k == "depth_pred":
            act[k] = torch.cat([1.0 / (torch.sigmoid(v[:, 0:1]) + 1e-12) - 1.0, v[:, 1:2]], 1)
        else:
            act[k] = v
    return raw, act
