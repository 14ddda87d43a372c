#!/usr/bin/env python
"""The fp32 exp results behind tests/golden/targets.npz: every Tensor.exp call the REAL reference's TargetGenerator
makes on that golden's input (the gaussian kernels of the heat-map splats), argument and result, one entry per distinct
argument.  torch's CPU exp goes through MKL's vector math, which dispatches by CPU vendor as well as instruction set, so
the last bit of a result depends on the host; with these the target test compares the oracle against the reference
bit for bit on any host.  Checks that the run reproduces targets.npz exactly before it writes anything.
Needs a checkout of the reference project (its path is the argument); the tests read tests/golden/targets_exp.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_targets_exp_golden.py <reference checkout>
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.abspath(sys.argv[1]))           # reference packages win name lookups
sys.path.append(os.path.join(REPO, "monocon-pytorch_amd"))

import numpy as np
import torch
from utils.target_generator import TargetGenerator          # noqa: E402  (reference)
from hipmonocon import synth                                # noqa: E402  (this repo)

SEED = 7
torch.set_num_threads(8)
# the input of targets.npz, as make_golden.py section (3) builds it
lab = synth.make_labels(SEED + 3, 3, 384, 1280)
lab["gt_bboxes"][2, 0] = [0.0, 100.0, 30.0, 380.0]
lab["gt_bboxes"][2, 1] = [1270.0, 370.0, 1279.0, 383.0]
lab["gt_kpts_2d"][2, 0, 0:4] = [-20.0, 50.0, 1300.0, 400.0]
lab["gt_kpts_valid_mask"][2, 0, 0:2] = 1
lab["mask"][2, 0:2] = 1
golden = np.load(os.path.join(HERE, "targets.npz"))
for k, v in lab.items():
    assert np.array_equal(v, golden["in." + k]), k

calls = []
real_exp = torch.Tensor.exp


def recording_exp(x):
    y = real_exp(x)
    a = x.detach().numpy().copy()
    if not any(c[0].shape == a.shape and np.array_equal(c[0].view(np.uint32), a.view(np.uint32)) for c in calls):
        calls.append((a, y.detach().numpy().copy()))
    return y


torch.Tensor.exp = recording_exp
try:
    data = {"img": torch.zeros(3, 3, 384, 1280), "img_metas": {"pad_shape": [(384, 1280)] * 3},
            "label": {k: torch.from_numpy(v.copy()) for k, v in lab.items()}}
    T = TargetGenerator()(data, feat_shape=(3, 64, 96, 320))
finally:
    torch.Tensor.exp = real_exp
for k, v in T.items():
    assert np.array_equal(v.numpy(), golden[k]), "this host does not reproduce targets.npz (%s)" % k
assert all(a.dtype == np.float32 for a, _ in calls)
out = {"n": np.int64(len(calls))}
for i, (a, y) in enumerate(calls):
    out["arg%d" % i], out["out%d" % i] = a, y
np.savez_compressed(os.path.join(HERE, "targets_exp.npz"), **out)
print("wrote targets_exp.npz: %d distinct exp arguments, shapes %s" % (len(calls), sorted({a.shape for a, _ in calls})))
