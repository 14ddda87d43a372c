"""LAMB on the GPU: ``mc_clip_lamb_step_classes`` / ``mc_lamb_ratios`` (csrc/kernels_optim.hip) against the float64 statement of
the formula (tests/lamb_reference.py), its determinism, the fused average, the guard, the argument checks, and the feature
through ``solver.AdamW(trust_ratio=True)`` and the engine (``SOLVER.LAMB``).

The table is the smallest at which the chunk walk, the tails and the per-tensor reduction can each go wrong -- 1, 3, 4, 65536,
65537, 131075 (three chunks, the last of 3 elements) and 200003 elements -- with one tensor all zeros (|p| = 0), one with zero
gradient, zero moments and no weight decay (|u| = 0) and one whose p, g, m and v all start one float into their allocations.
Classes: A adapts (weight decay), B does not (and maximizes), and -- one more than the two a parity run needs -- C, adapting
WITHOUT weight decay, because the |u| = 0 tensor must adapt for its ratio to be at stake and must not decay for u to vanish.

Tolerances.  Ratios: 2e-5 relative -- a lane adds at most 256 fp32 squares serially, then 8 tree levels and the LDS join,
<= 266 * 2^-24 ~ 1.6e-5 on a chunk sum; chunks are joined in double, each root halves it, two norms enter r.  m and v: 4 ulp
after the three steps; the ulp of v is that of its value (a sum of non-negative terms), the ulp of m is taken at the largest
magnitude that entered its sums over the run -- S_t = max(beta1 S_(t-1), |beta1 m| + |(1 - beta1) g'|), the error of an earlier
step decaying with beta1 like the value it sits in.  Where the two terms of m cancel, the value itself says nothing about the
rounding of its operands: the first run of this test found 4.48 ulp OF THE VALUE at one element of the 4-element tensor, whose
terms had cancelled at an earlier step; at S_t the run reads 3.30 ulp at worst (v: 3.03).
p: steps * (2e-5 * max |lr r u| + 2^-23 * max |p|) per tensor.
The clip coefficient of every step is formed from the norm the device wrote, in its float32 arithmetic (the global-norm pass is
not under test here and is only checked to agree with the float64 norm to 2e-5): a coefficient that differs in its last bits
would shift every g' -- and so m and v -- by more than the roundings this test is about.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import lamb_reference as R

pytestmark = pytest.mark.gpu

CHUNK = 65536
SIZES = (1, 3, 4, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 200003)
CLS = (0, 1, 0, 1, 2, 0, 0)
ZERO_P, ZERO_U, MISALIGNED = 2, 4, 5
N = len(SIZES)
ADAPT_MASK = 0b101
MAX_NORM = 5.0
STEPS = 3


def hyper(t):
    """the three classes at step index t (0-based): their own lr, betas, eps, weight decay and step count"""
    return [R.Hyper(1e-2, 0.9, 0.99, 1e-8, 1e-2, 2 + t, False, True),
            R.Hyper(3e-3, 0.8, 0.95, 1e-6, 5e-3, 7 + t, True, False),
            R.Hyper(2e-3, 0.9, 0.999, 1e-8, 0.0, 1 + t, False, True)]


def optim_classes(hp):
    from hipmonocon import lib as L
    return (L.OptimClass * len(hp))(*[(h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.step, 0, int(h.maximize)) for h in hp])


def misaligned(t):
    """a contiguous copy of ``t`` that starts one float into its storage: 4- but not 16-byte aligned"""
    buf = torch.zeros(t.numel() + 8, device="cuda", dtype=t.dtype)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.view(torch.int32)


def same_bits(xs, ys):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(xs, ys))


def ulp32(x):
    """the spacing of float32 at |x| (float64 array in, float64 out)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


@pytest.fixture(scope="module")
def data():
    """parameters, moments, averages and one gradient set per step, on the CPU; never modified"""
    gen = torch.Generator().manual_seed(17)
    p = [torch.randn(n, generator=gen) * 3 for n in SIZES]
    m = [torch.randn(n, generator=gen) * 0.01 for n in SIZES]
    v = [(torch.rand(n, generator=gen) + 0.5) * 1e-4 for n in SIZES]
    e = [torch.randn(n, generator=gen) for n in SIZES]
    g = [[torch.randn(n, generator=gen) * 3 for n in SIZES] for _ in range(STEPS)]
    p[ZERO_P].zero_()
    m[ZERO_U].zero_()
    v[ZERO_U].zero_()
    for t in range(STEPS):
        g[t][ZERO_U].zero_()
    return dict(p=p, m=m, v=v, e=e, g=g)


class Table:
    """the seven tensors with AdamW state, bound through the C ABI on a handle of their own"""

    def __init__(self, data, misalign=True, ema=False):
        from hipmonocon.engine import Engine
        self.eng = Engine(0)

        def put(t, i):
            return misaligned(t) if (misalign and i == MISALIGNED) else t.clone().cuda()

        self.data = data
        self.p, self.m, self.v = ([put(t, i) for i, t in enumerate(data[k])] for k in "pmv")
        self.g = [put(t, i) for i, t in enumerate(data["g"][0])]
        # averages: none for tensor 1, the one of the 65536-element tensor misaligned (whatever the rest is)
        self.e = [None if i == 1 else (misaligned(t) if i == 3 else t.clone().cuda()) for i, t in enumerate(data["e"])] if ema else None
        self.numel = (C.c_int64 * N)(*SIZES)
        self.norm = torch.zeros(1, device="cuda")

    def state(self):
        return self.p + self.m + self.v

    def bind(self, cls=CLS):
        rc = self.eng.lib.mc_optim_bind_classes(self.eng.h, N, ptr_array(self.p), ptr_array(self.g), ptr_array(self.m),
                                                ptr_array(self.v), None, self.numel, (C.c_int * N)(*cls))
        if rc == 0 and self.e is not None:
            rc = self.eng.lib.mc_optim_bind_ema(self.eng.h, N, ptr_array(self.e))
        return rc

    def set_grads(self, t):
        for dst, src in zip(self.g, self.data["g"][t]):
            dst.copy_(src)

    def step(self, t=0, hp=None, ncls=None, mask=ADAPT_MASK, trust_clip=0.0, max_norm=MAX_NORM, norm_type=2.0, w=0.0):
        hp = hyper(t) if hp is None else hp
        return self.eng.lib.mc_clip_lamb_step_classes(self.eng.h, optim_classes(hp), len(hp) if ncls is None else ncls, mask,
                                                      trust_clip, max_norm, norm_type, w, C.c_void_p(self.norm.data_ptr()), stream())

    def adamw_step(self, t=0):
        return self.eng.lib.mc_clip_adamw_step_classes(self.eng.h, optim_classes(hyper(t)), 3, MAX_NORM, 2.0, None, stream())

    def ratios(self, n=N):
        out = torch.full((max(n, 1),), -7.0, device="cuda")
        rc = self.eng.lib.mc_lamb_ratios(self.eng.h, C.c_void_p(out.data_ptr()), n, stream())
        return rc, out

    def run(self, steps=STEPS, **kw):
        assert self.bind() == 0, self.err()
        for t in range(steps):
            self.set_grads(t)
            assert self.step(t, **kw) == 0, self.err()
        torch.cuda.synchronize()
        rc, r = self.ratios()
        assert rc == 0, self.err()
        return r

    def err(self):
        return self.eng.lib.mc_last_error(self.eng.h).decode()


# ------------------------------------------------------------------------------------------------ 1. fp64 parity
def carry_scale(scale, ref, cls, hp):
    """S_t of the module docstring, per tensor (scale None: before the first step, whose inputs are exact)"""
    if scale is None:
        return list(ref.m_scale)
    return [np.maximum(hp[cls[i]].beta1 * scale[i], ref.m_scale[i]) for i in range(len(scale))]


def check_against_reference(p, m, v, ref, step_max, m_scale, what, steps=STEPS):
    """p, m, v: lists of device tensors; ref: the reference's last Result; step_max[i]: max |lr r u| over the steps; m_scale[i]:
    the magnitude the ulp of m is taken at (carry_scale)"""
    for i in range(len(p)):
        pi, mi, vi = (x.detach().cpu().double().numpy().ravel() for x in (p[i], m[i], v[i]))
        rp, rm, rv, ms = (np.asarray(x).ravel() for x in (ref.p[i], ref.m[i], ref.v[i], m_scale[i]))
        m_ulps = float((np.abs(mi - rm) / ulp32(np.maximum(np.abs(rm), ms))).max())
        v_ulps = float((np.abs(vi - rv) / ulp32(rv)).max())
        p_lim = steps * (2e-5 * step_max[i] + 2.0 ** -23 * float(np.abs(rp).max()))
        p_err = float(np.abs(pi - rp).max())
        print("%s tensor %d (numel %d): m within %.2f ulp, v within %.2f ulp, max |p - p64| = %.3e (bound %.3e)"
              % (what, i, pi.size, m_ulps, v_ulps, p_err, p_lim))
        assert m_ulps <= 4.0, (what, i, m_ulps)
        assert v_ulps <= 4.0, (what, i, v_ulps)
        assert p_err <= p_lim, (what, i, p_err, p_lim)


def test_three_steps_against_fp64(data):
    tab = Table(data)
    assert tab.bind() == 0, tab.err()
    p, m, v = ([t.double().numpy() for t in data[k]] for k in "pmv")
    step_max, m_scale = [0.0] * N, None
    for t in range(STEPS):
        tab.set_grads(t)
        assert tab.step(t) == 0, tab.err()
        torch.cuda.synchronize()
        g = [x.double().numpy() for x in data["g"][t]]
        norm, norm64 = float(tab.norm), R.total_norm(g)
        assert norm64 > MAX_NORM and abs(norm - norm64) <= 2e-5 * norm64, (norm, norm64)      # the clip is active
        ref = R.lamb_step(p, g, m, v, CLS, hyper(t), coef=R.clip_coef_f32(norm, MAX_NORM))
        rc, r = tab.ratios()
        assert rc == 0, tab.err()
        r = r.cpu().double().numpy()
        print("step %d ratios: device %s reference %s" % (t + 1, r.tolist(), ref.ratio))
        for i in range(N):
            assert abs(r[i] - ref.ratio[i]) <= 2e-5 * ref.ratio[i], (t, i, r[i], ref.ratio[i])
            if CLS[i] == 1 or (t == 0 and i in (ZERO_P, ZERO_U)):
                assert r[i] == 1.0, (t, i, r[i])            # not adapting, |p| = 0, |u| = 0: exactly 1
        p, m, v = ref.p, ref.m, ref.v
        step_max = [max(a, b) for a, b in zip(step_max, ref.step_max)]
        m_scale = carry_scale(m_scale, ref, CLS, hyper(t))
    assert any(abs(x - 1.0) > 0.1 for i, x in enumerate(ref.ratio) if CLS[i] != 1)      # the ratio does something here
    assert torch.equal(tab.p[ZERO_U].cpu(), data["p"][ZERO_U])                            # |u| = 0: p keeps every bit
    assert all(torch.equal(a.cpu(), b) for a, b in zip(tab.g, data["g"][-1]))            # the gradients are only read
    check_against_reference(tab.p, tab.m, tab.v, ref, step_max, m_scale, "C ABI")


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_same_bits_twice_and_whatever_the_alignment(data):
    a, b, c = Table(data), Table(data), Table(data, misalign=False)
    ra, rb, rc = a.run(), b.run(), c.run()
    assert a.p[MISALIGNED].data_ptr() % 16 == 4 and c.p[MISALIGNED].data_ptr() % 16 == 0
    assert same_bits(a.state(), b.state()) and torch.equal(bits(ra), bits(rb))
    assert same_bits(a.state(), c.state()) and torch.equal(bits(ra), bits(rc))
    assert not any(torch.equal(x.cpu(), y) for i, (x, y) in enumerate(zip(a.p, data["p"])) if i != ZERO_U)     # the steps did run


# ------------------------------------------------------------------------------------------------ 3. the LAMB signature
def test_adapting_tensors_move_by_lr_times_their_norm(data):
    tab = Table(data)
    r = tab.run(steps=1).cpu()
    hp = hyper(0)
    checked = 0
    for i in range(N):
        old, new = data["p"][i].double(), tab.p[i].cpu().double()
        if not hp[CLS[i]].adapts or float(old.norm()) == 0.0 or i == ZERO_U:      # (|u| = 0: r = 1 and nothing moves)
            continue
        moved = float((new - old).norm() / old.norm())
        print("tensor %d: |dp| / |p| = %.8g, lr = %g, r = %.6g" % (i, moved, hp[CLS[i]].lr, float(r[i])))
        assert abs(moved - hp[CLS[i]].lr) <= 1e-4 * hp[CLS[i]].lr, (i, moved)
        checked += 1
    assert checked == 3
    assert float(r.max()) > 1.0                     # ... so that the cap below has something to cap
    capped = Table(data).run(steps=1, trust_clip=1.0).cpu()
    assert float(capped.max()) <= 1.0 and bool((capped == torch.clamp(r, max=1.0)).all())


# ------------------------------------------------------------------------------------------------ 4. fused average
def test_fused_average_is_the_standalone_one_bit_for_bit(data):
    a, b = Table(data, ema=True), Table(data)
    ra, rb = a.run(w=0.25), b.run()
    assert same_bits(a.state(), b.state()) and torch.equal(bits(ra), bits(rb))        # attaching an average moves no bit
    assert a.e[3].data_ptr() % 16 == 4
    # the yardstick: mc_ema_update after every step, on a table of its own
    c = Table(data)
    e = [None if i == 1 else (misaligned(t) if i == 3 else t.clone().cuda()) for i, t in enumerate(data["e"])]
    idx = [i for i in range(N) if e[i] is not None]
    numel = (C.c_int64 * len(idx))(*[SIZES[i] for i in idx])
    assert c.bind() == 0
    assert c.eng.lib.mc_ema_bind(c.eng.h, len(idx), ptr_array([e[i] for i in idx]), ptr_array([c.p[i] for i in idx]), numel) == 0, c.err()
    for t in range(STEPS):
        c.set_grads(t)
        assert c.step(t) == 0 and c.eng.lib.mc_ema_update(c.eng.h, 0.25, stream()) == 0, c.err()
    torch.cuda.synchronize()
    assert same_bits(c.state(), a.state())
    assert same_bits([a.e[i] for i in idx], [e[i] for i in idx])
    assert not any(torch.equal(a.e[i].cpu(), data["e"][i]) for i in idx)


# ------------------------------------------------------------------------------------------------ 5. guard
def read_report(tab):
    from hipmonocon import lib as L
    dst = torch.zeros(C.sizeof(L.GuardReport), dtype=torch.uint8, device="cuda")
    assert tab.eng.lib.mc_optim_guard_report(tab.eng.h, C.c_void_p(dst.data_ptr()), stream()) == 0, tab.err()
    g = L.GuardReport.from_buffer_copy(bytes(dst.cpu().numpy()))
    return g.skipped, g.first_tensor, g.n_elements


def test_guarded_step(data):
    off, on = Table(data, ema=True), Table(data, ema=True)
    assert on.eng.lib.mc_optim_set_guard(on.eng.h, 1) == 0, on.err()
    r_off, r_on = off.run(steps=2, w=0.25), on.run(steps=2, w=0.25)
    e_ids = [i for i in range(N) if on.e[i] is not None]
    assert same_bits(off.state() + [off.e[i] for i in e_ids], on.state() + [on.e[i] for i in e_ids])
    assert torch.equal(bits(r_off), bits(r_on)) and read_report(on) == (0, -1, 0)
    # one NaN in the scalar tail of the last tensor's last chunk: nothing moves, the ratios included
    assert SIZES[6] % CHUNK % 4 == 3
    keep = [t.clone() for t in on.state() + [on.e[i] for i in e_ids]]
    on.set_grads(2)
    on.g[6][-1] = float("nan")
    rest = torch.randn(70000, device="cuda")            # the rest of an average: a table of its own
    rest_e, rest_keep = torch.zeros_like(rest), torch.zeros_like(rest)
    assert on.eng.lib.mc_ema_bind(on.eng.h, 1, ptr_array([rest_e]), ptr_array([rest]), (C.c_int64 * 1)(70000)) == 0, on.err()
    assert on.step(2, w=0.25) == 0, on.err()
    assert on.eng.lib.mc_ema_update_guarded(on.eng.h, 0.5, stream()) == 0, on.err()
    torch.cuda.synchronize()
    assert math.isnan(float(on.norm))
    assert same_bits(on.state() + [on.e[i] for i in e_ids], keep)
    rc, r_after = on.ratios()
    assert rc == 0 and torch.equal(bits(r_after), bits(r_on))
    assert read_report(on) == (1, 6, 1)
    assert torch.equal(rest_e, rest_keep)               # mc_ema_update_guarded did nothing
    # the next clean step is taken again, and the rest of the average follows
    on.set_grads(2)
    assert on.step(2, w=0.25) == 0 and on.eng.lib.mc_ema_update_guarded(on.eng.h, 0.5, stream()) == 0, on.err()
    torch.cuda.synchronize()
    assert read_report(on) == (0, -1, 0) and not torch.equal(on.p[6], keep[6]) and not torch.equal(rest_e, rest_keep)


# ------------------------------------------------------------------------------------------------ 6. argument checks
def test_argument_checks_fail_before_anything_is_launched(data):
    tab = Table(data, ema=True)
    keep = [t.clone() for t in tab.state()]
    nan, inf = float("nan"), float("inf")
    assert tab.step() != 0 and "bind" in tab.err()                                  # no table bound
    rc, _ = tab.ratios()
    assert rc != 0 and "mc_lamb_ratios" in tab.err()
    assert tab.bind() == 0, tab.err()
    rc, _ = tab.ratios()
    assert rc != 0 and "mc_clip_lamb_step_classes" in tab.err()                     # no LAMB step yet
    hp = hyper(0)
    assert tab.step(ncls=0) != 0 and tab.err()
    assert tab.step(hp=hp * 6, ncls=17) != 0 and "17" in tab.err()
    assert tab.step(hp=hp[:2], mask=0b01) != 0 and "class index 2" in tab.err()     # the table uses class 2
    assert tab.step(hp=[hp[0], hp[1]._replace(step=0), hp[2]]) != 0 and "step" in tab.err()
    for bad in (0.0, -1.0, nan):
        assert tab.step(norm_type=bad) != 0 and "norm_type" in tab.err(), bad
    from hipmonocon import lib as L
    ams = optim_classes(hp)
    ams[1].amsgrad = 1
    assert tab.eng.lib.mc_clip_lamb_step_classes(tab.eng.h, ams, 3, ADAPT_MASK, 0.0, MAX_NORM, 2.0, 0.0, None, stream()) != 0
    assert "amsgrad" in tab.err()
    assert tab.step(mask=0b1101) != 0 and "adapt_mask" in tab.err()
    for bad in (nan, inf, -1.0):
        assert tab.step(trust_clip=bad) != 0 and "trust_clip" in tab.err(), bad
    for bad in (nan, -0.1, 1.5):
        assert tab.step(w=bad) != 0 and "ema_weight" in tab.err(), bad
    rc, _ = tab.ratios()
    assert rc != 0                                                                  # none of the above counted as a step
    torch.cuda.synchronize()
    assert same_bits(tab.state(), keep)
    assert tab.step() == 0, tab.err()
    for n in (N - 1, N + 1, 0):
        rc, out = tab.ratios(n)
        assert rc != 0 and "mc_lamb_ratios" in tab.err(), n
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
    rc, out = tab.ratios()
    assert rc == 0 and bool((out > 0).all())
    assert tab.bind() == 0                                                          # a new table: its ratios are no step's
    rc, _ = tab.ratios()
    assert rc != 0
    assert L.OPT_MAX_CLASSES == 16


# ------------------------------------------------------------------------------------------------ 7. no residue
def test_adamw_after_lamb_is_adamw(data):
    a, b = Table(data), Table(data)
    a.run(steps=1)
    for dst, src in zip(a.state(), [t for k in "pmv" for t in data[k]]):
        dst.copy_(src)
    assert b.bind() == 0
    b.set_grads(0)
    assert a.adamw_step() == 0 and b.adamw_step() == 0, (a.err(), b.err())
    torch.cuda.synchronize()
    assert same_bits(a.state(), b.state())
    assert not torch.equal(b.p[0].cpu(), data["p"][0])


# ------------------------------------------------------------------------------------------------ 8. solver.AdamW
class Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, 8, 3, bias=True)
        self.bn = torch.nn.BatchNorm2d(8)
        self.conv2 = torch.nn.Conv2d(8, 16, 3, bias=False)


def small_optimizer(values, **kw):
    from solver import AdamW, build_param_groups
    net = Small().cuda()
    with torch.no_grad():
        for p, x in zip(net.parameters(), values):
            p.copy_(x)
    groups = build_param_groups(net.named_parameters(), lr=2e-3, weight_decay=1e-2, no_decay_norm_bias=True)
    assert len(groups) == 2 and groups[1]["weight_decay"] == 0.0
    return net, AdamW(groups, lr=2e-3, weight_decay=1e-2, betas=(0.9, 0.99), max_grad_norm=1.0, **kw)


def set_small_grads(net, grads):
    for p, g in zip(net.parameters(), grads):
        p.grad = g.clone().cuda()


def test_solver_adamw_with_trust_ratio():
    gen = torch.Generator().manual_seed(23)
    shapes = [tuple(p.shape) for p in Small().parameters()]
    values = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[torch.randn(s, generator=gen) for s in shapes] for _ in range(5)]
    net, opt = small_optimizer(values, trust_ratio=True)
    params = list(net.parameters())
    # the table order of step(): group 0 (decays: the two conv weights), then the no-decay group
    order = [p for g in opt.param_groups for p in g["params"]]
    pos = [next(i for i, q in enumerate(params) if q is p) for p in order]
    cls = [0 if p.dim() > 1 else 1 for p in order]
    assert cls == [0, 0, 1, 1, 1]
    p = [values[i].double().numpy() for i in pos]
    m, v = [np.zeros_like(x) for x in p], [np.zeros_like(x) for x in p]
    step_max, m_scale = [0.0] * len(p), None
    for t in range(3):
        set_small_grads(net, grads[t])
        opt.step()
        g = [grads[t][i].double().numpy() for i in pos]
        norm = float(opt.last_grad_norm)
        assert norm > 1.0 and abs(norm - R.total_norm(g)) <= 2e-5 * norm
        hp = [R.Hyper(2e-3, 0.9, 0.99, 1e-8, 1e-2, t + 1, False, True), R.Hyper(2e-3, 0.9, 0.99, 1e-8, 0.0, t + 1, False, False)]
        ref = R.lamb_step(p, g, m, v, cls, hp, coef=R.clip_coef_f32(norm, 1.0))
        p, m, v = ref.p, ref.m, ref.v
        step_max = [max(a, b) for a, b in zip(step_max, ref.step_max)]
        m_scale = carry_scale(m_scale, ref, cls, hp)
        ratios = opt.trust_ratios()
        assert list(ratios) == order
        for i, q in enumerate(order):
            assert abs(ratios[q] - ref.ratio[i]) <= 2e-5 * ref.ratio[i], (t, i)
            assert (ratios[q] == 1.0) == (cls[i] == 1), (t, i, ratios[q])          # 1 for the no-decay group, and only there
        assert list(opt.trust_ratios(adapting_only=True)) == order[:2]
    check_against_reference(order, [opt.state[q]["exp_avg"] for q in order], [opt.state[q]["exp_avg_sq"] for q in order],
                            ref, step_max, m_scale, "solver.AdamW")
    assert set(opt.state[order[0]]) == {"step", "exp_avg", "exp_avg_sq"} and float(opt.state[order[0]]["step"]) == 3.0
    # a state_dict() round trip into a fresh optimizer: the next step is bit-identical
    net2, opt2 = small_optimizer([q.detach().cpu() for q in params], trust_ratio=True)
    opt2.load_state_dict(opt.state_dict())
    for o, n in ((opt, net), (opt2, net2)):
        set_small_grads(n, grads[3])
        o.step()
    torch.cuda.synchronize()
    assert same_bits([q.detach() for q in net.parameters()], [q.detach() for q in net2.parameters()])
    assert opt.trust_ratios() != {} and list(opt.trust_ratios().values()) == list(opt2.trust_ratios().values())
    # trust_ratio off: the AdamW entry again -- the bits of a plain optimizer that loads the same state
    net3, opt3 = small_optimizer([q.detach().cpu() for q in params])
    opt3.load_state_dict(opt.state_dict())
    assert opt3._adapts() is None
    opt.trust_ratio = False
    for o, n in ((opt, net), (opt3, net3)):
        set_small_grads(n, grads[4])
        o.step()
    torch.cuda.synchronize()
    assert same_bits([q.detach() for q in net.parameters()], [q.detach() for q in net3.parameters()])
    for q, q3 in zip(net.parameters(), net3.parameters()):
        assert same_bits([opt.state[q][k] for k in ("exp_avg", "exp_avg_sq")], [opt3.state[q3][k] for k in ("exp_avg", "exp_avg_sq")])


# ------------------------------------------------------------------------------------------------ 9. engine
def engine_cfg(out_dir, lamb):
    from utils.engine_utils import get_default_cfg
    cfg = get_default_cfg()
    cfg.set_new_allowed(True)
    cfg.OUTPUT_DIR = str(out_dir)
    cfg.SEED = 3
    cfg.DATA.ROOT = 'synthetic'
    cfg.DATA.SYNTHETIC_LENGTH = 4
    cfg.DATA.SYNTHETIC_HW = [96, 224]
    cfg.DATA.BATCH_SIZE = 2
    cfg.DATA.NUM_WORKERS = 0
    cfg.MODEL.BACKBONE.IMAGENET_PRETRAINED = False
    cfg.SOLVER.OPTIM.NUM_EPOCHS = 2
    # |p_new - p| = lr |p| is read off float32 parameters, each rounded by up to 2^-24 |p|: against a step of lr |p| that is
    # 6e-8 / lr per element, which only averages out over many elements.  1e-2 keeps a 1-element tensor within 6e-6 of lr.
    cfg.SOLVER.OPTIM.LR = 1e-2
    cfg.SOLVER.LAMB.ENABLE = lamb
    cfg.PERIOD.EVAL_PERIOD = 0
    cfg.PERIOD.LOG_PERIOD = 1
    return cfg


def test_engine_trains_with_lamb_and_its_checkpoint_loads_without(tmp_path, capsys):
    from engine.monocon_engine import MonoconEngine
    from utils.engine_utils import set_random_seed
    set_random_seed(3)
    on, off = os.path.join(tmp_path, "on"), os.path.join(tmp_path, "off")
    os.makedirs(on), os.makedirs(off)
    eng = MonoconEngine(engine_cfg(on, True))
    opt = eng.optimizer
    assert (opt.trust_ratio, opt.trust_clip, opt.always_adapt) == (True, 0.0, False) and opt._adapts() == [True]
    # every step: the parameters and the learning rate before it, the parameters after it
    shots = []
    opt.register_step_pre_hook(lambda o, a, k: shots.append([o.param_groups[0]["lr"], {p: p.detach().clone() for p in o.param_groups[0]["params"]}]))
    opt.register_step_post_hook(lambda o, a, k: shots[-1].append({p: p.detach().clone() for p in o.param_groups[0]["params"]}))
    eng.train_one_epoch()
    torch.cuda.synchronize()
    assert len(shots) == 2 and len(eng.entire_losses) == 2 and all(math.isfinite(x) for x in eng.entire_losses)
    assert "Trust ratio" in capsys.readouterr().out
    ratios = opt.trust_ratios()
    checked = 0
    for lr, before, after in shots:
        for p in ratios:                                   # the parameters the step bound: those with a gradient
            old, new = before[p].double(), after[p].double()
            if float(old.norm()) == 0.0:
                continue
            moved = float((new - old).norm() / old.norm())
            assert abs(moved - lr) <= 1e-4 * lr, (tuple(p.shape), moved, lr)
            checked += 1
    assert checked > 100 and shots[0][0] != shots[1][0]                         # (the schedule moved lr between the steps)
    eng.save_checkpoint(post_fix='t')
    path = os.path.join(on, 'checkpoints', 'epoch_001_t.pth')
    d = torch.load(path, weights_only=False)
    assert all("trust_ratio" not in g for g in d['state_dict']['optimizer']['param_groups'])
    plain = MonoconEngine(engine_cfg(off, False))
    assert plain.optimizer.trust_ratio is False
    plain.load_checkpoint(path)
    assert plain.optimizer._adapts() is None and plain.epochs == eng.epochs
    for (k, a), b in zip(eng.model.state_dict().items(), plain.model.state_dict().values()):
        assert torch.equal(a, b), k
    for pa, pb in zip(eng.model.parameters(), plain.model.parameters()):
        sa, sb = opt.state.get(pa, {}), plain.optimizer.state.get(pb, {})
        assert set(sa) == set(sb)
        assert all(torch.equal(sa[k].cpu(), sb[k].cpu()) for k in sa)
