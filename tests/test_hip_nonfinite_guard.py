"""The fused AdamW's non-finite guard (``mc_optim_set_guard``, ``solver.AdamW(skip_nonfinite=True)``,
``SOLVER.NONFINITE_GUARD``) on the GPU.

1. guard on + finite gradients == guard off, bit for bit, on every bound buffer;
2. a step whose gradient norm is not finite writes nothing, reports the culprit, and still counts;
3. five steps with steps 2 and 4 poisoned against ``torch.optim.AdamW`` + ``clip_grad_norm_`` in float64 on the CPU that
   skips those two steps (without the guard the same sequence leaves NaN in parameters, moments and average for good);
4. argument and state checks of the C entries and of ``clip_grad_norm_(error_if_nonfinite=...)``;
5. the engine: a run with one poisoned step finishes, logs it by parameter name, keeps everything finite, checkpoints the count.

The tensor set is ``BIG + 2100 x (5,)`` of test_optim_groups.py (more chunks than workgroups, a tensor across the 65536-element
chunk boundary, a single element, a gradient at element offset 1), in its two groups -- here one amsgrad, one maximize.  The
table the kernels walk is group 0 then group 1; ``Side.table`` is that order.  NaN / +inf / -inf are planted where the walk can
go wrong (``PLACES``).  Non-finite values are ordinary data for these element-wise kernels: nothing here does more than place
them in tensors.
"""
import ctypes as C
import math
import os

import pytest
import torch

from conftest import rel_err
from test_hip_model_ema import Raw, engine_cfg, misaligned, ptr_array, snapshot, stream
from test_optim_groups import BIG, HYPER, MISALIGNED, N_ALL, N_SMALL, NORM_TOL, TOL, device_grad, two_groups

pytestmark = pytest.mark.gpu

CHUNK = 65536
SHAPES = BIG + [(5,)] * N_SMALL
EMA_MISALIGNED = 3                  # the (10, 64) tensor's average starts one float into its storage
NAN, INF = math.nan, math.inf


def table_order():
    g0, g1 = two_groups()
    return g0 + g1


def second_chunk_tensor():
    """a five-element tensor that a workgroup reaches as its SECOND chunk: the table has 2107 chunks (the 70000-element tensor,
    third in the table, has two), the launch 2048 workgroups, so workgroup 10 walks chunk 10 and then chunk 2058, which is the
    tensor at table position 2057"""
    i = table_order()[2058 - 1]
    assert SHAPES[i] == (5,)
    return i


# (tensor, flat element, value).  The 70000-element tensor's last chunk is elements 65536..69999: 4464 = 4 * 1116 of them, so
# when everything is 16-byte aligned that chunk is all float4 body and its last element is the body's last lane; the scalar
# TAIL of an aligned chunk is elements 128..130 of the 131-element tensor, and the whole misaligned tensor is walked by scalars.
PLACES = {
    "body": (0, 1001, NAN),                         # float4 body of the first tensor
    "last_chunk": (4, 69999, INF),                  # the end of the last chunk of the tensor that crosses the chunk boundary
    "tail": (1, 130, -INF),                         # scalar tail of an aligned chunk
    "misaligned": (MISALIGNED, 36, -INF),           # gradient at element offset 1
    "second_chunk": (second_chunk_tensor(), 2, INF),
}
POISONS = {
    "all": tuple(PLACES),
    "second_chunk_only": ("second_chunk",),
    "last_chunk_and_misaligned": ("last_chunk", "misaligned"),
    "tail_only": ("tail",),
}


@pytest.fixture(scope="module")
def data():
    """(initial values, gradients, running statistics) on the CPU and a cache of the gradients on the device per scale; the
    device gradients are shared by every optimizer of a test -- the step only reads them, which test 2 checks"""
    gen = torch.Generator().manual_seed(0)
    base = [torch.randn(s, generator=gen) for s in SHAPES]
    grads = [torch.randn(s, generator=gen) * 3 for s in SHAPES]
    stats = torch.randn(CHUNK + 9, generator=gen)
    cache = {}

    def on_device(scale):
        if scale not in cache:
            cache[scale] = [device_grad(g * scale, i == MISALIGNED) for i, g in enumerate(grads)]
        return cache[scale]

    return base, grads, stats, on_device


def poisoned(data, scale, names):
    """the device gradients at ``scale`` with the values of ``names`` planted (the poisoned tensors are fresh copies)"""
    out = list(data[3](scale))
    for name in names:
        i, off, val = PLACES[name]
        g = data[1][i] * scale
        g.view(-1)[off] = val
        out[i] = device_grad(g, i == MISALIGNED)
    return out


class Net(torch.nn.Module):
    def __init__(self, values):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(v.clone().cuda()) for v in values])
        self.frozen = torch.nn.Parameter(torch.linspace(-1, 1, 1031).cuda())        # never gets a gradient
        self.register_buffer("running_mean", torch.zeros(CHUNK + 9, device="cuda"))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long, device="cuda"))


class Side:
    """the fused optimizer over the set, on a handle of its own: two groups (one amsgrad, one maximize with its own lr) or
    ``plain`` (one group without flags: the reference recipe's kernels), with or without a ModelEMA of the model"""

    def __init__(self, data, guard, ema=True, max_norm=5.0, norm_type=2.0, plain=False):
        from hipmonocon.engine import Engine
        from solver import AdamW, ModelEMA
        self.data = data
        self.net = Net(data[0])
        w = list(self.net.w)
        if plain:
            self.table = list(range(N_ALL))
            groups = [dict(params=w)]
        else:
            g0, g1 = two_groups()
            self.table = g0 + g1
            groups = [dict(params=[w[i] for i in g0], amsgrad=True), dict(params=[w[i] for i in g1], maximize=True, lr=3e-3)]
        self.opt = AdamW(groups, max_grad_norm=max_norm, norm_type=norm_type, skip_nonfinite=guard, engine=Engine(0), **HYPER)
        self.ema = None
        if ema:
            self.ema = ModelEMA(self.net, decay=0.9, warmup=True)
            k = "w.%d" % EMA_MISALIGNED
            self.ema.tensors[k] = misaligned(self.ema.tensors[k])
            self.opt.set_ema(self.ema)

    def step(self, grads, scale):
        for p, g in zip(self.net.w, grads):
            p.grad = g
        self.net.running_mean.copy_(self.data[2] * scale)       # what a train-mode forward does to the buffers
        self.net.num_batches_tracked.add_(1)
        self.opt.step()

    def buffers(self):
        """every float tensor the step may write, by name: p, m, v, vmax, the fused and the update_rest averages, out_norm"""
        out = {"out_norm": self.opt.last_grad_norm}
        for i, p in enumerate(self.net.w):
            out["p%d" % i] = p.detach()
            for k, t in self.opt.state.get(p, {}).items():
                if k != "step":
                    out["%s%d" % (k, i)] = t
        if self.ema is not None:
            out.update(("ema." + k, t) for k, t in self.ema.tensors.items() if t.is_floating_point())
        return out


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def assert_same_bits(a, b):
    """two name -> tensor maps hold the same bits (one comparison over everything; per tensor only to name a difference)"""
    assert a.keys() == b.keys()
    if torch.equal(torch.cat([bits(t).reshape(-1) for t in a.values()]), torch.cat([bits(t).reshape(-1) for t in b.values()])):
        return
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k


# ------------------------------------------------------------------------------------------------ 1. guard on, finite gradients
CASES_1 = [(p, m, True, False) for p in (2.0, 1.0, math.inf, 3.0) for m in (None, 5.0)] + \
          [(2.0, 5.0, False, False), (2.0, 5.0, True, True), (2.0, None, False, True)]


@pytest.mark.parametrize("norm_type,max_norm,ema,plain", CASES_1)
def test_guard_on_with_finite_gradients_is_the_unguarded_step_bit_for_bit(data, norm_type, max_norm, ema, plain):
    off = Side(data, False, ema, max_norm, norm_type, plain)
    on = Side(data, True, ema, max_norm, norm_type, plain)
    for it in range(3):
        grads = data[3](it + 1)
        off.step(grads, it + 1)
        on.step(grads, it + 1)
        assert torch.equal(bits(on.opt.last_grad_norm), bits(off.opt.last_grad_norm)), it
    torch.cuda.synchronize()
    a, b = off.buffers(), on.buffers()
    assert len(a) == 1 + N_ALL * 3 + (N_ALL + 1) // 2 * (0 if plain else 1) + ((N_ALL + 2) if ema else 0)
    assert_same_bits(a, b)
    assert not torch.equal(on.net.w[0].detach().cpu(), data[0][0])                  # ... and the steps did run
    recs = on.opt.drain_guard_reports(keep=0)
    assert [(r.step, r.skipped, r.param, r.n_elements) for r in recs] == [(1, False, None, 0), (2, False, None, 0), (3, False, None, 0)]
    assert [bits(torch.tensor(r.norm)).item() for r in recs][-1] == bits(on.opt.last_grad_norm).item()
    assert on.opt.skipped_steps == 0 and off.opt.skipped_steps == 0 and off.opt.drain_guard_reports(keep=0) == []
    if ema:
        assert on.ema.updates == off.ema.updates == 3
        assert not torch.equal(on.ema.tensors["running_mean"], on.net.running_mean)     # an average, not a copy


# ------------------------------------------------------------------------------------------------ 2. a skipped step
@pytest.mark.parametrize("which", sorted(POISONS))
@pytest.mark.parametrize("norm_type,plain", ((2.0, False), (math.inf, False), (2.0, True)))
def test_a_skipped_step_writes_nothing_and_names_the_culprit(data, which, norm_type, plain):
    s = Side(data, True, True, 5.0, norm_type, plain)
    s.step(data[3](1), 1)                                       # a taken step first: every state tensor exists and is non-zero
    with torch.no_grad():                                       # a signed zero is a bit pattern too
        s.net.w[1][0] = -0.0
        s.opt.state[s.net.w[0]]["exp_avg"].view(-1)[5] = -0.0
        s.ema.tensors["w.2"][0] = -0.0
        s.ema.tensors["running_mean"][7] = -0.0
    names = POISONS[which]
    grads = poisoned(data, 2, names)
    before = {k: t.clone() for k, t in s.buffers().items() if k != "out_norm"}
    grads_before = [g.clone() for g in grads]
    steps_before = [float(s.opt.state[p]["step"]) for p in s.net.w]
    s.step(grads, 2)
    torch.cuda.synchronize()
    after = s.buffers()
    norm = float(after.pop("out_norm"))
    assert_same_bits(before, after)
    for i, (g, h) in enumerate(zip(grads, grads_before)):       # the gradients are only read
        assert torch.equal(bits(g), bits(h)), i
    values = [PLACES[n][2] for n in names]
    assert not math.isfinite(norm)
    if norm_type == math.inf:
        assert math.isnan(norm) if any(v != v for v in values) else norm == INF
    recs = s.opt.drain_guard_reports(keep=0)
    assert [(r.step, r.skipped) for r in recs] == [(1, False), (2, True)]
    first = min((PLACES[n][0] for n in names), key=s.table.index)
    assert recs[1].param is s.net.w[first], (s.table.index(first), which)
    assert recs[1].n_elements == len(names)
    assert math.isnan(recs[1].norm) if math.isnan(norm) else recs[1].norm == norm
    assert s.opt.skipped_steps == 1
    # it still counts: the step, the average's updates, the integer entry of the average
    assert [float(s.opt.state[p]["step"]) for p in s.net.w] == [x + 1 for x in steps_before]
    assert s.ema.updates == 2 and int(s.ema.tensors["num_batches_tracked"]) == 2
    # ... and the next finite step is taken
    s.step(data[3](3), 3)
    torch.cuda.synchronize()
    assert math.isfinite(float(s.opt.last_grad_norm))
    later = s.buffers()
    for k in ("p0", "exp_avg4", "ema.w.0", "ema.running_mean", "p%d" % second_chunk_tensor()):
        assert not torch.equal(bits(later[k]), bits(before[k])), k
    assert all(bool(torch.isfinite(t).all()) for t in later.values())
    assert [r.skipped for r in s.opt.drain_guard_reports(keep=0)] == [False]


@pytest.mark.parametrize("plain", (False, True))
def test_a_norm_that_overflows_from_finite_gradients_is_skipped_without_a_culprit(data, plain):
    """1e20 squared is past fp32: the L2 norm as computed is inf although every element is finite -- skipped, as
    clip_grad_norm_(error_if_nonfinite=True) judges it, with nothing to name.  The inf-norm of the same input is 1e20: taken."""
    for norm_type, skipped in ((2.0, True), (math.inf, False)):
        s = Side(data, True, True, 5.0, norm_type, plain)
        s.step(data[3](1), 1)
        grads = list(data[3](2))
        g = data[1][4] * 2
        g[66000] = 1e20
        grads[4] = g.cuda()
        before = {k: t.clone() for k, t in s.buffers().items() if k != "out_norm"}
        s.step(grads, 2)
        torch.cuda.synchronize()
        after = s.buffers()
        norm = float(after.pop("out_norm"))
        rec = s.opt.drain_guard_reports(keep=0)[1]
        if skipped:
            assert norm == INF
            assert_same_bits(before, after)
            assert (rec.skipped, rec.param, rec.n_elements, rec.norm) == (True, None, 0, INF)
        else:
            assert norm == pytest.approx(1e20, rel=1e-6)
            assert (rec.skipped, rec.param, rec.n_elements) == (False, None, 0)
            assert not torch.equal(bits(after["p0"]), bits(before["p0"]))
        assert s.opt.skipped_steps == int(skipped)


# ------------------------------------------------------------------------------------------------ 3. five steps against fp64
def test_five_steps_two_of_them_poisoned_against_fp64(data):
    """The behavioural proof: steps 2 and 4 carry NaN / inf gradients.  The reference -- torch.optim.AdamW + clip_grad_norm_ on
    float64 CPU copies -- does not step on them and adds 1 to every state['step'] (a skipped step counts).  Tolerances: the
    project's own for three taken steps (TOL, NORM_TOL of test_optim_groups.py).  Without the guard the poisoned elements are
    NaN for good after step 2 (the next test)."""
    s = Side(data, True, True, 5.0, 2.0)
    g0, g1 = two_groups()
    ref = [torch.nn.Parameter(v.double()) for v in data[0]]
    opt = torch.optim.AdamW([dict(params=[ref[i] for i in g0], amsgrad=True), dict(params=[ref[i] for i in g1], maximize=True, lr=3e-3)],
                            **HYPER)
    poison = {2: POISONS["all"], 4: POISONS["second_chunk_only"]}
    for it in range(1, 6):
        s.step(poisoned(data, it, poison[it]) if it in poison else data[3](it), it)
        if it in poison:
            assert not math.isfinite(float(s.opt.last_grad_norm)), it
            for st in opt.state.values():
                st["step"] += 1
            continue
        for p, g in zip(ref, data[1]):
            p.grad = g.double() * it
        ref_norm = torch.nn.utils.clip_grad_norm_(ref, 5.0, norm_type=2.0)
        opt.step()
        assert float(s.opt.last_grad_norm) == pytest.approx(float(ref_norm), rel=NORM_TOL), it
    torch.cuda.synchronize()
    worst = {}
    for i, (p, q) in enumerate(zip(s.net.w, ref)):
        sa, sb = s.opt.state[p], opt.state[q]
        assert set(sa) == set(sb), i
        assert float(sa["step"]) == float(sb["step"]) == 5.0, i
        for k, a, b in [("param", p, q)] + [(k, sa[k], sb[k]) for k in sb if k != "step"]:
            e = rel_err(a, b)
            worst[k] = max(worst.get(k, 0.0), e)
            assert e < TOL, (k, i, e)
    print("five steps, two skipped, worst rel_err against fp64: " + ", ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert [r.skipped for r in s.opt.drain_guard_reports(keep=0)] == [False, True, False, True, False]
    assert s.opt.skipped_steps == 2 and s.ema.updates == 5
    assert all(bool(torch.isfinite(t).all()) for t in s.buffers().values())


def test_without_the_guard_the_same_gradients_destroy_the_run(data):
    """what the guard is for, on the same input: the norm is NaN, the coefficient therefore 1, and the element that meets the
    NaN is NaN from then on -- in the parameter, in both moments and in the weight average (max_exp_avg_sq is an fmaxf and
    keeps its finite value)"""
    s = Side(data, False, True, 5.0, 2.0)
    s.step(data[3](1), 1)
    s.step(poisoned(data, 2, ("body",)), 2)
    s.step(data[3](3), 3)                                       # finite gradients again: too late
    torch.cuda.synchronize()
    i, off, _ = PLACES["body"]
    st = s.opt.state[s.net.w[i]]
    for t in (s.net.w[i], st["exp_avg"], st["exp_avg_sq"], s.ema.tensors["w.%d" % i]):
        assert math.isnan(float(t.detach().view(-1)[off]))
    assert s.opt.skipped_steps == 0 and s.opt.drain_guard_reports(keep=0) == []


# ------------------------------------------------------------------------------------------------ 4. arguments and state
def set_guard(r, on):
    return r.eng.lib.mc_optim_set_guard(r.eng.h, on)


def report(r, dst):
    return r.eng.lib.mc_optim_guard_report(r.eng.h, dst, stream())


def read_report(r):
    from hipmonocon import lib as L
    dst = torch.zeros(C.sizeof(L.GuardReport), dtype=torch.uint8, device="cuda")
    assert report(r, C.c_void_p(dst.data_ptr())) == 0, r.err()
    g = L.GuardReport.from_buffer_copy(bytes(dst.cpu().numpy()))
    return g.skipped, g.first_tensor, g.n_elements, g.norm


def test_guard_off_after_on_restores_the_old_entries():
    a, b = Raw(), Raw()
    for r in (a, b):
        assert r.bind() == 0 and r.bind_ema() == 0, r.err()
    assert set_guard(b, 1) == 0 and set_guard(b, 1) == 0            # (on twice is on)
    assert read_report(b) == (0, -1, 0, 0.0)                        # before the first guarded step
    assert a.ema_step(0.25) == 0 and b.ema_step(0.25) == 0, b.err()
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a.all(), b.all()))
    rep = read_report(b)
    assert rep[:3] == (0, -1, 0) and rep[3] > 5.0
    assert set_guard(b, 0) == 0
    assert report(b, C.c_void_p(a.p[0].data_ptr())) != 0 and "guard is off" in b.err()
    assert a.step() == 0 and b.step() == 0 and a.ema_step(0.5) == 0 and b.ema_step(0.5) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a.all(), b.all()))
    # the original single-recipe entry under the guard: mc_optim_bind + mc_clip_adamw_step
    c, d = Raw(), Raw()
    for r in (c, d):
        assert r.eng.lib.mc_optim_bind(r.eng.h, r.n, ptr_array(r.p), ptr_array(r.g), ptr_array(r.m), ptr_array(r.v), r.numel) == 0
    assert set_guard(d, 1) == 0
    keep = [t.clone() for t in d.all()]
    d.g[0][CHUNK + 4] = NAN                                         # the scalar tail of the second chunk of tensor 0
    for r in (c, d):
        assert r.eng.lib.mc_clip_adamw_step(r.eng.h, 1e-3, 0.9, 0.99, 1e-8, 1e-2, 5.0, 3, None, stream()) == 0, r.err()
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(d.p + d.m + d.v, keep[:3] + keep[6:12]))
    rep = read_report(d)
    assert rep[:3] == (1, 0, 1) and math.isnan(rep[3])
    d.g[0][CHUNK + 4] = c.g[0][CHUNK + 4]
    assert d.eng.lib.mc_clip_adamw_step(d.eng.h, 1e-3, 0.9, 0.99, 1e-8, 1e-2, 5.0, 3, None, stream()) == 0, d.err()
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(c.all(), d.all()))
    assert read_report(d)[:3] == (0, -1, 0)


def test_ema_update_guarded_follows_the_last_guarded_step():
    a, b = Raw(), Raw()
    src = [t.clone() + 1 for t in a.p]
    for r in (a, b):
        assert r.bind() == 0, r.err()
        assert r.eng.lib.mc_ema_bind(r.eng.h, 3, ptr_array(r.e), ptr_array(src), r.numel) == 0, r.err()
    start = [t.clone() for t in a.e]
    # guard off, and guard on with no guarded step behind it: mc_ema_update
    assert a.eng.lib.mc_ema_update(a.eng.h, 0.25, stream()) == 0
    assert b.eng.lib.mc_ema_update_guarded(b.eng.h, 0.25, stream()) == 0, b.err()
    assert a.eng.lib.mc_ema_update(a.eng.h, 0.5, stream()) == 0
    assert set_guard(b, 1) == 0
    assert b.eng.lib.mc_ema_update_guarded(b.eng.h, 0.5, stream()) == 0, b.err()
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a.e, b.e))
    assert not any(torch.equal(x, y) for x, y in zip(b.e, start))
    # after a skipped step it does nothing; after a taken one it is mc_ema_update again
    held = [t.clone() for t in b.e]
    good = b.g[1][3].clone()
    b.g[1][3] = -INF
    assert b.step() == 0
    assert b.eng.lib.mc_ema_update_guarded(b.eng.h, 0.5, stream()) == 0, b.err()
    torch.cuda.synchronize()
    assert read_report(b)[:3] == (1, 1, 1)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(b.e, held))
    b.g[1][3] = good
    assert b.step() == 0 and b.eng.lib.mc_ema_update_guarded(b.eng.h, 0.5, stream()) == 0
    assert a.eng.lib.mc_ema_update(a.eng.h, 0.5, stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a.e, b.e))
    for bad in (float("nan"), -0.1, 1.5):
        assert b.eng.lib.mc_ema_update_guarded(b.eng.h, bad, stream()) != 0 and "ema_weight" in b.err(), bad
    c = Raw()
    assert set_guard(c, 1) == 0 and c.bind() == 0 and c.step() == 0
    assert c.eng.lib.mc_ema_update_guarded(c.eng.h, 0.5, stream()) != 0 and "mc_ema_bind" in c.err()


def test_a_bad_report_destination_fails_before_anything_is_enqueued():
    from hipmonocon import lib as L
    r = Raw()
    assert r.bind() == 0
    assert report(r, C.c_void_p(r.p[0].data_ptr())) != 0 and "guard is off" in r.err()
    assert set_guard(r, 1) == 0 and r.step() == 0
    torch.cuda.synchronize()
    keep = [t.clone() for t in r.all()]
    assert report(r, None) != 0 and "bad argument" in r.err()
    pageable = L.GuardReport(7, 7, 7, 7.0)
    assert report(r, C.c_void_p(C.addressof(pageable))) != 0 and "page-locked" in r.err()
    torch.cuda.synchronize()
    assert (pageable.skipped, pageable.first_tensor, pageable.n_elements, pageable.norm) == (7, 7, 7, 7.0)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(r.all(), keep))
    pinned = torch.zeros(C.sizeof(L.GuardReport), dtype=torch.uint8, pin_memory=True)
    assert report(r, C.c_void_p(pinned.data_ptr())) == 0, r.err()
    torch.cuda.synchronize()
    g = L.GuardReport.from_address(pinned.data_ptr())
    assert (g.skipped, g.first_tensor, g.n_elements) == (0, -1, 0) and g.norm > 0


def test_clip_grad_norm_error_if_nonfinite(data):
    from solver import clip_grad_norm_
    ids = list(range(12))

    def params(grads):
        ps = [torch.nn.Parameter(torch.zeros(SHAPES[i], device="cuda")) for i in ids]
        for p, g in zip(ps, grads):
            p.grad = g
        return ps

    finite = [data[3](1)[i].clone() for i in ids]
    a, b, c = params([g.clone() for g in finite]), params([g.clone() for g in finite]), params([g.clone() for g in finite])
    na = clip_grad_norm_(a, 5.0)
    nb = clip_grad_norm_(b, 5.0, error_if_nonfinite=False)
    nc = clip_grad_norm_(c, 5.0, error_if_nonfinite=True)           # a finite norm: the clip of always
    assert torch.equal(bits(na), bits(nb)) and torch.equal(bits(na), bits(nc)) and float(na) > 5.0
    for p, q, r, g in zip(a, b, c, finite):
        assert torch.equal(bits(p.grad), bits(q.grad)) and torch.equal(bits(p.grad), bits(r.grad))
        assert not torch.equal(p.grad, g)
    for value in (NAN, INF, -INF):
        bad = [g.clone() for g in finite]
        bad[4].view(-1)[69999] = value
        ps = params(bad)
        held = [g.clone() for g in bad]
        with pytest.raises(RuntimeError, match="non-finite, so it cannot be clipped"):
            clip_grad_norm_(ps, 5.0, error_if_nonfinite=True)
        assert all(torch.equal(bits(p.grad), bits(h)) for p, h in zip(ps, held))
        n = clip_grad_norm_(ps, 5.0)                                 # as today: the non-finite norm, returned
        assert not math.isfinite(float(n))


# ------------------------------------------------------------------------------------------------ 5. engine
def guard_cfg(out_dir, max_consecutive=10):
    cfg = engine_cfg(out_dir, True)
    cfg.SOLVER.NONFINITE_GUARD.ENABLE = True
    cfg.SOLVER.NONFINITE_GUARD.MAX_CONSECUTIVE = max_consecutive
    return cfg


def poison_steps(eng, when, seen):
    """wrap optimizer.step: on the iterations ``when`` selects, write inf into one named parameter's gradient first"""
    step = eng.optimizer.step

    def wrapped(*a, **k):
        if when(eng.global_iters):
            name, p = [(n, q) for n, q in eng.model.named_parameters() if q.grad is not None][40]
            p.grad.view(-1)[0] = INF
            seen.append(name)
        return step(*a, **k)

    eng.optimizer.step = wrapped


def test_engine_survives_a_poisoned_step_and_checkpoints_the_count(tmp_path, capsys):
    from engine.monocon_engine import MonoconEngine
    from utils.engine_utils import set_random_seed
    set_random_seed(3)
    out = os.path.join(tmp_path, "run")
    os.makedirs(out)
    eng = MonoconEngine(guard_cfg(out))
    assert eng.optimizer.skip_nonfinite and eng.skipped_steps == 0 and eng.max_consecutive_skips == 10
    seen = []
    poison_steps(eng, lambda it: it == 2, seen)
    eng.train()
    torch.cuda.synchronize()
    text = capsys.readouterr().out
    assert len(seen) == 1
    line = [l for l in text.splitlines() if "SKIPPED" in l]
    assert len(line) == 1 and "Iteration 2:" in line[0] and "'%s'" % seen[0] in line[0] and "1 non-finite element" in line[0], text
    assert eng.skipped_steps == 1 and eng.optimizer.skipped_steps == 1 and eng.consecutive_skips == 0
    assert eng.global_iters == 5 and len(eng.entire_losses) == 3          # four steps, the skipped one's loss left out
    assert all(math.isfinite(x) for x in eng.entire_losses)
    assert all(bool(torch.isfinite(v).all()) for v in eng.model.state_dict().values())
    assert all(bool(torch.isfinite(v).all()) for v in eng.ema.tensors.values() if v.is_floating_point())
    assert eng.ema.updates == 4 and {int(st["step"]) for st in eng.optimizer.state.values()} == {4}      # it counted
    d = torch.load(os.path.join(out, "checkpoints", "epoch_002_final.pth"), weights_only=False)
    assert d["engine_attrs"]["skipped_steps"] == 1
    eng2 = MonoconEngine(guard_cfg(out))                                # auto-resume finds the file
    assert eng2.skipped_steps == 1 and eng2.consecutive_skips == 0 and eng2.optimizer.skip_nonfinite


def test_engine_gives_up_after_max_consecutive_skipped_steps(tmp_path, capsys):
    from engine.monocon_engine import MonoconEngine
    from utils.engine_utils import set_random_seed
    set_random_seed(3)
    out = os.path.join(tmp_path, "run")
    os.makedirs(out)
    eng = MonoconEngine(guard_cfg(out, max_consecutive=2))
    before = snapshot(eng.model)
    seen = []
    poison_steps(eng, lambda it: True, seen)
    with pytest.raises(RuntimeError, match="2 optimizer steps in a row"):
        eng.train_one_epoch()
    torch.cuda.synchronize()
    assert len(seen) == 2 and eng.skipped_steps == 2 and eng.entire_losses == []
    assert capsys.readouterr().out.count("SKIPPED") == 2
    for k, v in eng.model.named_parameters():                           # no step was taken
        assert torch.equal(bits(v), bits(before[k])), k
