"""The image-gradient golden (tests/golden/img_grad.npz, make_img_grad_golden.py) and the two entry points behind img.grad,
without a GPU."""
import os
import re

import numpy as np

from conftest import REPO, load_golden

CASES = (0, 1)
FIELDS = ("seed", "shape", "g64", "gnorm64", "gerr32", "gerr32_1t", "gmargin")


def test_golden_loads_and_matches_the_pinned_fixtures():
    """the two cases are the flip-free fixtures train_cond_0 / train_cond_1 pin: same seeds, same shapes"""
    g = load_golden("img_grad.npz")
    assert sorted(g.files) == sorted("c%d.%s" % (c, f) for c in CASES for f in FIELDS)
    for c, (seed, shape) in zip(CASES, ((417, (4, 64, 64)), (423, (8, 32, 64)))):
        pin = load_golden("train_cond_%d.npz" % c)
        assert int(g["c%d.seed" % c]) == int(pin["seed"]) == seed
        assert tuple(int(v) for v in g["c%d.shape" % c]) == tuple(int(v) for v in pin["shape"]) == shape
        B, H, W = shape
        g64 = g["c%d.g64" % c]
        assert g64.shape == (B, 3, H, W) and g64.dtype == np.float32 and g64.size == 49152
        assert np.isfinite(g64).all() and not (g64 == 0).any()
        # the stored float32 values carry the fp64 norm to float32 precision
        assert abs(float(np.linalg.norm(g64.astype(np.float64))) - float(g["c%d.gnorm64" % c])) <= 1e-6 * float(g["c%d.gnorm64" % c])
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "img_grad.npz")) < 1 << 20


def test_recorded_reference_errors_are_below_the_makers_limits():
    """cond_train's acceptance, on the image gradient: perturbed fp64 < 1e-4, the reference's own fp32 (8 threads and 1)
    < 2e-4 -- and 100x inside the 1e-3 gate of the GPU test"""
    g = load_golden("img_grad.npz")
    for c in CASES:
        assert 0 < float(g["c%d.gmargin" % c]) < 1e-4
        assert 0 < float(g["c%d.gerr32" % c]) < 2e-4 and 0 < float(g["c%d.gerr32_1t" % c]) < 2e-4
        assert max(float(g["c%d.gerr32" % c]), float(g["c%d.gerr32_1t" % c])) < 1e-3 / 50


def test_the_new_entry_points_exist_in_header_and_binding():
    from hipmonocon import lib
    txt = open(os.path.join(REPO, "include", "monocon_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("mc_backward_image_grad", "mc_op_stem_dgrad", "mc_op_stem_dgrad_fused"):
        assert re.search(r"\bint %s\s*\(" % name, txt), name
        assert name in lib.EXPORTS, name
    if os.path.exists(lib.LIB_PATH):
        l = lib.load()
        assert l.mc_backward_image_grad.argtypes is not None and len(l.mc_backward_image_grad.argtypes) == 5
        assert len(l.mc_op_stem_dgrad.argtypes) == 8 and len(l.mc_op_stem_dgrad_fused.argtypes) == 10
