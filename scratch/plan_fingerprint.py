"""Fingerprint of the train plan for one precision mode and the MONOCON_HIP_* switches of the environment it is started
with: two optimiser steps on the golden state at B = 4, 128x224 and at B = 2, 384x1280, printed as ONE JSON line with
workspace_bytes() and the SHA-256 of the losses, of every parameter gradient after step 1 and of every parameter and
buffer after step 2.  Two builds of the library that plan the same launches print the same line, byte for byte.

    python scratch/plan_fingerprint.py f16x2            # MONOCON_HIP_LAZY_Z=0 python scratch/plan_fingerprint.py f16x2
"""
import hashlib, json, os, sys
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "monocon-pytorch_amd"), REPO):
    sys.path.insert(0, p)
from hipmonocon import synth
from model import MonoConDetector
from solver import AdamW

mode = sys.argv[1] if len(sys.argv) > 1 else "f16x2"
stats = np.load(os.path.join(REPO, "tests", "golden", "bn_calib_seed7.npz"))


def digest(named):
    h = hashlib.sha256()
    for name, t in named:
        h.update(name.encode())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def run(B, H, W):
    sd = synth.make_state_dict(7, bn_stats={k: stats[k] for k in stats.files})
    m = MonoConDetector(34, pretrained_backbone=False)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train().set_precision(mode)
    opt = AdamW(m.parameters(), lr=2.25e-4, weight_decay=1e-5, betas=(0.95, 0.99), max_grad_norm=35.0)
    b = synth.make_batch(500, B, H, W)
    bt = {"img": b["img"].cuda().contiguous(), "label": {k: v.cuda().contiguous() for k, v in b["label"].items()},
          "img_metas": {"pad_shape": [(H, W)] * B}}
    losses, grads = [], None
    for step in range(2):
        opt.zero_grad()
        _, loss = m(bt)
        sum(loss.values()).backward()
        torch.cuda.synchronize()
        losses += [("%d.%s" % (step, k), v) for k, v in sorted(loss.items())]
        if step == 0:
            grads = digest((n, p.grad) for n, p in m.named_parameters() if p.grad is not None)
        opt.step()
    torch.cuda.synchronize()
    return {"shape": [B, H, W], "workspace_bytes": m._rt.engine.workspace_bytes(), "losses": digest(losses), "grads_step1": grads,
            "state_step2": digest(sorted(m.state_dict().items()))}


switches = {k: v for k, v in sorted(os.environ.items()) if k.startswith("MONOCON_HIP_") and k != "MONOCON_HIP_TUNE_CACHE"}
print(json.dumps({"mode": mode, "switches": switches, "runs": [run(4, 128, 224), run(2, 384, 1280)]}, sort_keys=True))
