"""LAMB without a device: the float64 yardstick (tests/lamb_reference.py) pinned to ``torch.optim.AdamW`` where no class
adapts and to a hand-computed case where some do, the SOLVER.LAMB keys, the constructor's checks and the class folding of a
LAMB step."""
import inspect
import math

import numpy as np
import pytest
import torch

import lamb_reference as R


def test_reference_without_adapting_classes_is_torch_adamw():
    """3 steps, two groups (their own lr, betas, eps, weight decay), a clip that is active: 1e-12 relative"""
    gen = torch.Generator().manual_seed(2)
    shapes = [(7, 5), (33,), (4, 3, 2), (1,)]
    cls = [0, 1, 0, 1]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in shapes]
    groups = [dict(params=params[0::2], lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2),
              dict(params=params[1::2], lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.0)]
    opt = torch.optim.AdamW(groups)
    p = [q.detach().numpy().copy() for q in params]
    m = [np.zeros_like(x) for x in p]
    v = [np.zeros_like(x) for x in p]
    max_norm = 2.0
    for t in range(1, 4):
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * 3 for s in shapes]
        for q, g in zip(params, grads):
            q.grad = g.clone()
        norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        assert norm > max_norm                                       # the clip is active
        opt.step()
        g = [x.numpy() for x in grads]
        assert math.isclose(R.total_norm(g), norm, rel_tol=1e-14)
        classes = [R.Hyper(1e-3, 0.9, 0.99, 1e-8, 1e-2, t), R.Hyper(3e-3, 0.8, 0.95, 1e-6, 0.0, t)]
        res = R.lamb_step(p, g, m, v, cls, classes, coef=R.clip_coef(R.total_norm(g), max_norm))
        p, m, v = res.p, res.m, res.v
        assert res.ratio == [1.0] * 4
        for i, q in enumerate(params):
            st = opt.state[q]
            for mine, theirs in ((p[i], q.detach().numpy()), (m[i], st["exp_avg"].numpy()), (v[i], st["exp_avg_sq"].numpy())):
                err = np.abs(mine - theirs).max() / np.abs(theirs).max()
                assert err <= 1e-12, (t, i, err)


def test_reference_ratio_by_hand():
    """two tensors, zero moments, step 1, eps 0, no clip: m = (1 - b1) g, v = (1 - b2) g^2, so m / bc1 = g and
    sqrt(v) / sqrt(bc2) = |g|: the Adam part of u is sign(g).  With wd 0.5: u = sign(g) + p / 2."""
    hp = R.Hyper(0.1, 0.9, 0.99, 0.0, 0.5, 1, False, True)
    p = [np.array([3.0, -4.0]), np.array([2.0, 0.0, 0.0])]
    g = [np.array([1.0, 2.0]), np.array([-5.0, 1.0, 1.0])]
    zeros = [np.zeros(2), np.zeros(3)]
    res = R.lamb_step(p, g, zeros, zeros, [0, 0], [hp])
    u0, u1 = np.array([1.0 + 1.5, 1.0 - 2.0]), np.array([-1.0 + 1.0, 1.0, 1.0])
    r0, r1 = 5.0 / math.sqrt(2.5 ** 2 + 1.0), 2.0 / math.sqrt(2.0)
    assert math.isclose(res.ratio[0], r0, rel_tol=1e-13) and math.isclose(res.ratio[1], r1, rel_tol=1e-13)
    assert np.allclose(res.p[0], p[0] - 0.1 * r0 * u0, rtol=1e-13, atol=0) and np.allclose(res.p[1], p[1] - 0.1 * r1 * u1, rtol=1e-13, atol=0)
    # the LAMB signature: |p_new - p| = lr |p|
    assert math.isclose(np.linalg.norm(res.p[0] - p[0]), 0.1 * 5.0, rel_tol=1e-14)
    # trust_clip caps the ratio; a class that does not adapt has r = 1
    capped = R.lamb_step(p, g, zeros, zeros, [0, 0], [hp], trust_clip=1.0)
    assert capped.ratio == [1.0, 1.0]                               # both r0 and r1 exceed 1
    part = R.lamb_step(p, g, zeros, zeros, [0, 0], [hp], trust_clip=1.6).ratio
    assert part[0] == 1.6 and math.isclose(part[1], r1, rel_tol=1e-13)
    assert R.lamb_step(p, g, zeros, zeros, [0, 0], [hp._replace(adapts=False)]).ratio == [1.0, 1.0]
    # |p| = 0 -> r = 1
    z = R.lamb_step([np.zeros(2), p[1]], g, zeros, zeros, [0, 0], [hp])
    assert z.ratio[0] == 1.0 and np.allclose(z.p[0], -0.1 * np.array([1.0, 1.0]), rtol=1e-13, atol=0)
    # |u| = 0 (no gradient, no moments, no decay) -> r = 1 and p stays, instead of |p| / 0
    s = R.lamb_step(p, [np.zeros(2), g[1]], zeros, zeros, [0, 0], [hp._replace(weight_decay=0.0, eps=1e-8)])
    assert s.ratio[0] == 1.0 and np.array_equal(s.p[0], p[0])
    # a NaN norm: the comparisons are false, r = 1, the NaN reaches p through u
    n = R.lamb_step(p, [np.array([np.nan, 1.0]), g[1]], zeros, zeros, [0, 0], [hp])
    assert n.ratio[0] == 1.0 and np.isnan(n.p[0][0])
    # maximize flips the gradient's sign after the clip coefficient
    mx = R.lamb_step(p, g, zeros, zeros, [0, 0], [hp._replace(maximize=True)], coef=0.5)
    mn = R.lamb_step(p, [-x for x in g], zeros, zeros, [0, 0], [hp], coef=0.5)
    assert all(np.array_equal(a, b) for a, b in zip(mx.p + mx.m + mx.v, mn.p + mn.m + mn.v))
    # the average follows the NEW parameters
    e = R.lamb_step(p, g, zeros, zeros, [0, 0], [hp], e=[np.ones(2), None], ema_weight=0.25)
    assert np.allclose(e.e[0], 1.0 + 0.25 * (res.p[0] - 1.0), rtol=1e-13) and e.e[1] is None


def test_config_defaults():
    from utils.engine_utils import get_default_cfg
    c = get_default_cfg()
    assert c.SOLVER.LAMB.ENABLE is False and c.SOLVER.LAMB.TRUST_CLIP == 0.0 and c.SOLVER.LAMB.ALWAYS_ADAPT is False
    assert set(c.SOLVER.LAMB.keys()) == {"ENABLE", "TRUST_CLIP", "ALWAYS_ADAPT"}


def test_constructor_validation_and_defaults():
    from solver import AdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    sig = inspect.signature(AdamW.__init__).parameters
    assert sig["trust_ratio"].default is False and sig["trust_clip"].default == 0.0 and sig["always_adapt"].default is False
    opt = AdamW(p)
    assert (opt.trust_ratio, opt.trust_clip, opt.always_adapt) == (False, 0.0, False) and opt._adapts() is None
    assert "trust_ratio" not in opt.state_dict()["param_groups"][0]          # torch's checkpoint layout is untouched
    assert type(AdamW(p, trust_ratio=True)).__name__ == "AdamW"                # CyclicScheduler asserts on the name
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="trust_clip"):
            AdamW(p, trust_ratio=True, trust_clip=bad)
    with pytest.raises(ValueError, match="amsgrad"):
        AdamW(p, trust_ratio=True, amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        AdamW([dict(params=p, trust_ratio=True)], amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        AdamW([dict(params=p, amsgrad=True)], trust_ratio=True)
    opt = AdamW(p, trust_ratio=True)
    q = [torch.nn.Parameter(torch.zeros(2))]
    with pytest.raises(ValueError, match="amsgrad"):
        opt.add_param_group(dict(params=q, amsgrad=True))
    with pytest.raises(ValueError, match="amsgrad"):                        # one launch steps every group: none may be amsgrad
        opt.add_param_group(dict(params=q, amsgrad=True, trust_ratio=False))
    with pytest.raises(ValueError, match="amsgrad"):
        AdamW(p, amsgrad=True).add_param_group(dict(params=q, trust_ratio=True, amsgrad=False))
    assert len(opt.param_groups) == 1                                       # the refused groups were not added
    opt.add_param_group(dict(params=q, trust_ratio=False))
    assert len(opt.param_groups) == 2 and opt._adapts() == [True, False]
    with pytest.raises(Exception, match="trust_ratios"):
        opt.trust_ratios()                                                  # no LAMB step has run


def test_which_groups_adapt():
    from solver import AdamW
    a, b, c = ([torch.nn.Parameter(torch.zeros(2))] for _ in range(3))
    groups = [dict(params=a), dict(params=b, weight_decay=0.0), dict(params=c, trust_ratio=False)]
    assert AdamW(groups, weight_decay=1e-2)._adapts() is None
    assert AdamW(groups, weight_decay=1e-2, trust_ratio=True)._adapts() == [True, False, False]
    assert AdamW(groups, weight_decay=1e-2, trust_ratio=True, always_adapt=True)._adapts() == [True, True, False]
    per_group = [dict(params=a), dict(params=b, trust_ratio=True)]
    assert AdamW(per_group, weight_decay=1e-2)._adapts() == [False, True]
    # load_state_dict keeps the optimizer's own mode: an AdamW file into a LAMB optimizer and back
    lamb, plain = AdamW(per_group, weight_decay=1e-2), AdamW([dict(params=a), dict(params=b)], weight_decay=1e-2)
    lamb.load_state_dict(plain.state_dict())
    assert lamb._adapts() == [False, True]
    plain.load_state_dict(AdamW(per_group, weight_decay=1e-2).state_dict())
    assert plain._adapts() is None and all("trust_ratio" not in g for g in plain.param_groups)


def test_lamb_class_folding():
    from hipmonocon.lib import MonoconHipError
    from solver.fused_adamw import MAX_CLASSES, class_key, fold_classes, fold_lamb_classes
    base = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
    groups = [dict(base), dict(base), dict(base, weight_decay=0.0), dict(base, lr=2e-3)]
    adapts = [True, False, False, True]
    # groups 0 and 1 differ in nothing but the adapt bit: AdamW folds them into one class, LAMB into two
    pairs = [(1, 5), (0, 5), (2, 5), (1, 5), (3, 5), (0, 6), (0, 5)]
    assert len(fold_classes(groups, pairs)[0]) == 4
    classes, cls, mask = fold_lamb_classes(groups, pairs, adapts)
    assert cls == (0, 1, 2, 0, 3, 4, 1)                                     # first-appearance order
    assert classes == [class_key(groups[1], 5), class_key(groups[0], 5), class_key(groups[2], 5), class_key(groups[3], 5),
                       class_key(groups[0], 6)]
    assert all(len(k) == 8 for k in classes)                                # mc_optim_class rows, the adapt bit rides in the mask
    assert mask == 0b11010
    assert fold_lamb_classes(groups, pairs, [False] * 4)[2] == 0
    # more than MAX_CLASSES classes raise: 9 step counts x 2 adapt bits
    many = [(gi, s) for s in range(1, 10) for gi in (0, 1)]
    assert len(fold_classes(groups, many)[0]) == 9
    with pytest.raises(MonoconHipError, match=str(MAX_CLASSES)):
        fold_lamb_classes(groups, many, adapts)
    assert len(fold_lamb_classes(groups, many[:MAX_CLASSES], adapts)[0]) == MAX_CLASSES
