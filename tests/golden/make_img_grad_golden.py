#!/usr/bin/env python
"""Golden image gradients: d sum(loss_dict.values()) / d img of the REAL reference, on the two flip-free fixtures that
train_cond_0.npz (4x64x64, seed 417) and train_cond_1.npz (8x32x64, seed 423) already pin.

Runs only in the build container (needs /root/reference, read-only), like make_golden.py, whose `ref_model` / `save` it
imports.  State and batch come from hipmonocon.synth; only reference OUTPUTS are stored, in tests/golden/img_grad.npz.  Per
case c:

    c<c>.seed, c<c>.shape   copied from train_cond_<c>.npz (the seeds are fixed by the committed goldens, never re-drawn)
    c<c>.g64                the fp64 gradient wrt the image, stored as float32 (B,3,H,W)
    c<c>.gnorm64            its fp64 norm
    c<c>.gerr32             the reference's own fp32-vs-fp64 relative L2, 8 threads
    c<c>.gerr32_1t          the same with 1 thread
    c<c>.gmargin            relative L2 between the fp64 gradient and the fp64 gradient of the image perturbed by 3e-7
                            relative noise (cond_train's margin test, the same noise stream)

The script asserts cond_train's own acceptance on the image gradient (perturbed < 1e-4, fp32 < 2e-4) and aborts otherwise.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_img_grad_golden.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np                                          # noqa: E402
import torch                                                # noqa: E402

from make_golden import META, SEED, ref_model, save         # noqa: E402  (puts the reference and hipmonocon on the path)
from hipmonocon import synth                                # noqa: E402

MARGIN_LIMIT, FP32_LIMIT = 1e-4, 2e-4                       # cond_train's acceptance
CASES = (0, 1)


def image_grad(sd, batch, double, img=None):
    m = ref_model(sd, train=True, double=double)
    b = dict(batch)
    x = b["img"] if img is None else img
    x = (x.double() if double else x.float()).clone().requires_grad_(True)
    b["img"] = x
    _, loss = m(b)
    sum(loss.values()).backward()
    return x.grad.detach().double()


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def main():
    stats = np.load(os.path.join(HERE, "bn_calib_seed7.npz"))
    sd = synth.make_conditioned_state_dict(SEED, bn_stats={k: stats[k] for k in stats.files})
    out = {}
    for case in CASES:
        pin = np.load(os.path.join(HERE, "train_cond_%d.npz" % case))
        seed, (B, H, W) = int(pin["seed"]), [int(v) for v in pin["shape"]]
        b = synth.make_conditioned_batch(seed, B, H, W)
        g64 = image_grad(sd, b, True)
        noise = torch.from_numpy(synth.uniform(seed, "cond.noise", tuple(b["img"].shape), -1.0, 1.0))
        margin = rel_l2(image_grad(sd, b, True, b["img"].double() * (1.0 + 3e-7 * noise)), g64)
        e32 = rel_l2(image_grad(sd, b, False), g64)
        torch.set_num_threads(1)
        e32_1t = rel_l2(image_grad(sd, b, False), g64)
        torch.set_num_threads(META["threads"])
        print("image gradient case %d: B=%d %dx%d seed %d  norm %.4g  perturbed-fp64 %.2e  ref fp32-vs-fp64 %.2e (8 threads) / %.2e (1)"
              "  exact zeros %d" % (case, B, H, W, seed, float(g64.norm()), margin, e32, e32_1t, int((g64 == 0).sum())))
        assert margin < MARGIN_LIMIT, "case %d: the image gradient moves %.1e under 3e-7 noise" % (case, margin)
        assert max(e32, e32_1t) < FP32_LIMIT, "case %d: the reference's fp32 image gradient is %.1e off its fp64 one" % (case, max(e32, e32_1t))
        p = "c%d." % case
        out.update({p + "seed": seed, p + "shape": np.array([B, H, W]), p + "g64": g64.float(), p + "gnorm64": g64.norm(),
                    p + "gerr32": e32, p + "gerr32_1t": e32_1t, p + "gmargin": margin})
    save("img_grad.npz", **out)


if __name__ == "__main__":
    main()
