"""The LAMB step of include/monocon_hip.h (``mc_clip_lamb_step_classes``) stated in float64 numpy: the yardstick of
tests/test_lamb_host.py (which pins it to ``torch.optim.AdamW`` where no class adapts) and of tests/test_hip_lamb.py.

Per tensor, with the hyper-parameters of its class and t = the class's 1-based step::

    g' = coef * g                      (coef: the clip coefficient, negated for a maximize class)
    m  = beta1 m + (1 - beta1) g'
    v  = beta2 v + (1 - beta2) g'^2
    u  = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd * p        bc1 = 1 - beta1^t, bc2 = 1 - beta2^t
    r  = |p| / |u|  if the class adapts and |p| > 0 and |u| > 0, else 1;  r = min(r, trust_clip) if trust_clip > 0
    p  = p - lr * r * u;               e = e + w (p - e) where an average is attached and w > 0
"""
import collections

import numpy as np

Hyper = collections.namedtuple("Hyper", "lr beta1 beta2 eps weight_decay step maximize adapts")
Hyper.__new__.__defaults__ = (False, False)

Result = collections.namedtuple("Result", "p m v e ratio step_max m_scale")
Result.__doc__ = """new p, m, v, e (lists of float64 arrays; e entries may be None), the ratios, and per tensor max |lr r u| and
the element-wise magnitude |beta1 m| + |(1 - beta1) g'| that entered m (the scale its rounding error is measured at)"""


def total_norm(grads, norm_type=2.0):
    g = [np.asarray(x, dtype=np.float64).ravel() for x in grads]
    if norm_type == float("inf"):
        return max(float(np.abs(x).max()) for x in g)
    return float(sum(float((np.abs(x) ** norm_type).sum()) for x in g) ** (1.0 / norm_type))


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient in float64"""
    if not max_norm > 0.0:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


def clip_coef_f32(norm, max_norm):
    """the coefficient exactly as the final norm kernel forms it, in float32 from the float32 norm it wrote"""
    if not max_norm > 0.0:
        return 1.0
    c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return float(c) if c < np.float32(1.0) else 1.0


def lamb_step(p, g, m, v, cls, classes, coef=1.0, trust_clip=0.0, e=None, ema_weight=0.0):
    """one step over lists of arrays; ``cls[i]`` indexes ``classes`` (``Hyper`` rows).  Nothing is modified in place."""
    P, M, V, E, R, S, MS = [], [], [], [], [], [], []
    for i in range(len(p)):
        hp = classes[cls[i]]
        pi, gi, mi, vi = (np.asarray(x, dtype=np.float64) for x in (p[i], g[i], m[i], v[i]))
        gc = (-coef if hp.maximize else coef) * gi
        t1, t2 = hp.beta1 * mi, (1.0 - hp.beta1) * gc
        mn = t1 + t2
        vn = hp.beta2 * vi + (1.0 - hp.beta2) * gc * gc
        bc1, bc2 = 1.0 - hp.beta1 ** hp.step, 1.0 - hp.beta2 ** hp.step
        u = (mn / bc1) / (np.sqrt(vn) / np.sqrt(bc2) + hp.eps) + hp.weight_decay * pi
        pn, un = float(np.sqrt((pi * pi).sum())), float(np.sqrt((u * u).sum()))
        r = pn / un if (hp.adapts and pn > 0.0 and un > 0.0) else 1.0
        if trust_clip > 0.0:
            r = min(r, trust_clip)
        new_p = pi - hp.lr * r * u
        P.append(new_p); M.append(mn); V.append(vn); R.append(r)
        S.append(float(np.abs(hp.lr * r * u).max()))
        MS.append(np.abs(t1) + np.abs(t2))
        ei = None if e is None or e[i] is None else np.asarray(e[i], dtype=np.float64)
        if ei is not None and ema_weight > 0.0:
            ei = ei + ema_weight * (new_p - ei)
        E.append(ei)
    return Result(P, M, V, E, R, S, MS)
