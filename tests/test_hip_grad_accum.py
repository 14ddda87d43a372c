"""Gradient accumulation on the GPU: ``mc_accum_bind`` / ``mc_grad_accumulate`` (csrc/kernels_optim.hip) bit for bit against
separate torch operations on the device, ``solver.GradAccumulator`` in front of the fused step and its guard, the detector's
train step accumulated over a window, the deferred gradient exchange on a world-1 communicator, and ``SOLVER.ACCUM_STEPS``
through the engine.

The tensor set is the optimizer tests': more chunks than the launch has workgroups (2107 against 2048), a 70000-element tensor
across the 65536-element chunk boundary, a 131-element tensor whose last three elements are the scalar tail, a single element,
and a gradient that starts one float into its storage.

Every comparison is of BITS: the arithmetic is fixed as one fp32 round-to-nearest add per micro-batch and one fp32
round-to-nearest multiply by float32(1 / k) at the end, which is what the torch operations of the references perform.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import GOLDEN_SEED
from hipmonocon import dist as hdist
from hipmonocon import synth
from test_hip_comm import build, step, to_cuda
from test_hip_model_ema import ptr_array, stream
from test_hip_nonfinite_guard import PLACES, Side, assert_same_bits
from test_optim_groups import BIG, MISALIGNED, N_SMALL, device_grad

pytestmark = pytest.mark.gpu

SHAPES = BIG + [(5,)] * N_SMALL
N = len(SHAPES)
SENTINEL = 7.25
K_MAX = 5


def f32(x):
    """``x`` rounded to float32, as a Python float: what the kernel multiplies by"""
    return float(np.float32(x))


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def sets():
    """K_MAX distinct random gradient sets on the device (plain, aligned tensors); never modified"""
    gen = torch.Generator().manual_seed(21)
    return [[(torch.randn(s, generator=gen) * (1 + j)).cuda() for s in SHAPES] for j in range(K_MAX)]


@pytest.fixture(scope="module")
def torch_windows(sets):
    """k -> (sum of the first k - 1 sets, mean of the k sets), formed by separate torch operations on the device"""
    out = {}
    for k in (2, 3, 5):
        a = [g.clone() for g in sets[0]]
        for j in range(1, k - 1):
            for x, g in zip(a, sets[j]):
                x += g
        s = f32(1.0 / k)
        out[k] = (a, [(x + g) * s for x, g in zip(a, sets[k - 1])])
    return out


class Buffers:
    """gradient and accumulator buffers for the set.  ``g_off`` / ``a_off``: tensor index -> element offset of the view in its
    storage (missing: 0).  The gradients live in buffers of their own (zero around the view); the accumulators in ONE flat
    buffer filled with a sentinel, every slice at a multiple of 4 floats plus its offset"""

    def __init__(self, g_off=None, a_off=None):
        g_off, a_off = g_off or {}, a_off or {}
        self.gbuf, self.g = [], []
        for i, s in enumerate(SHAPES):
            n = math.prod(s)
            buf = torch.zeros(n + 8, device="cuda")
            o = g_off.get(i, 0)
            self.gbuf.append(buf)
            self.g.append(buf[o:o + n].view(s))
        starts, total = [], 0
        for i, s in enumerate(SHAPES):
            starts.append(total + a_off.get(i, 0))
            total += (math.prod(s) + 3) // 4 * 4 + (4 if a_off.get(i, 0) else 0)
        self.flat = torch.full((total,), SENTINEL, device="cuda")
        self.a = [self.flat[o:o + math.prod(s)] for o, s in zip(starts, SHAPES)]
        self.mask = torch.zeros(total, dtype=torch.bool, device="cuda")       # True: an accumulator element
        for o, s in zip(starts, SHAPES):
            self.mask[o:o + math.prod(s)] = True
        assert all(t.is_contiguous() for t in self.g + self.a)

    def load(self, grads):
        torch._foreach_copy_(self.g, list(grads))

    def window(self, eng, sets, k):
        from hipmonocon.lib import ACCUM_ADD, ACCUM_BEGIN, ACCUM_FINISH
        for j in range(k):
            self.load(sets[j])
            eng.grad_accumulate(ACCUM_BEGIN if j == 0 else ACCUM_FINISH if j == k - 1 else ACCUM_ADD, 1.0 / k)
        torch.cuda.synchronize()

    def untouched_around(self):
        """the accumulator buffer outside the slices keeps the sentinel, the gradient buffers outside the views their zeros"""
        assert bool((self.flat[~self.mask] == SENTINEL).all())
        for buf, g in zip(self.gbuf, self.g):
            o = (g.data_ptr() - buf.data_ptr()) // 4
            assert not bool(buf[:o].any()) and not bool(buf[o + g.numel():].any())


# ------------------------------------------------------------------------------------------------ 1. against torch, bit for bit
@pytest.mark.parametrize("acc_misaligned", (False, True), ids=("acc_aligned", "acc_offset_1"))
@pytest.mark.parametrize("k", (2, 3, 5))
def test_window_equals_separate_torch_operations_bit_for_bit(sets, torch_windows, k, acc_misaligned):
    from hipmonocon.engine import Engine
    eng = Engine(0)
    b = Buffers(g_off={MISALIGNED: 1}, a_off={MISALIGNED: 1} if acc_misaligned else None)
    assert b.g[MISALIGNED].data_ptr() % 16 == 4 and b.a[MISALIGNED].data_ptr() % 16 == (4 if acc_misaligned else 0)
    assert all(a.data_ptr() % 16 == 0 for i, a in enumerate(b.a) if i != MISALIGNED)
    eng.accum_bind(b.g, b.a)
    b.window(eng, sets, k)
    ref_sum, ref_mean = torch_windows[k]
    for i in range(N):
        assert bits_equal(b.g[i], ref_mean[i]), ("mean", i, SHAPES[i])
        assert bits_equal(b.a[i].view(SHAPES[i]), ref_sum[i]), ("sum of the first k - 1", i, SHAPES[i])
    b.untouched_around()
    # the same table, the next window: BEGIN overwrites what the last one left
    b.window(eng, sets[1:], 2)
    assert all(bits_equal(b.g[i], (sets[1][i] + sets[2][i]) * 0.5) for i in range(N))
    assert all(bits_equal(b.a[i].view(SHAPES[i]), sets[1][i]) for i in range(N))
    b.untouched_around()


# ------------------------------------------------------------------------------------------------ 2. body / tail independence
def test_bits_do_not_depend_on_body_tail_or_alignment(sets, torch_windows):
    from hipmonocon.engine import Engine
    eng = Engine(0)
    every = {i: 1 for i in range(N)}
    aligned, shifted = Buffers(), Buffers(g_off=every, a_off=every)
    assert all(t.data_ptr() % 16 == 0 for t in aligned.g + aligned.a)
    assert all(t.data_ptr() % 16 == 4 for t in shifted.g + shifted.a)
    for b in (aligned, shifted):
        eng.accum_bind(b.g, b.a)
        b.window(eng, sets, 3)
        b.untouched_around()
    for i in range(N):
        assert bits_equal(aligned.g[i], shifted.g[i]) and bits_equal(aligned.a[i], shifted.a[i]), (i, SHAPES[i])
        assert bits_equal(aligned.g[i], torch_windows[3][1][i]), (i, SHAPES[i])


# ------------------------------------------------------------------------------------------------ 3. in front of the fused step
@pytest.fixture(scope="module")
def guard_data():
    """the (values, gradients, statistics, device cache) tuple that test_hip_nonfinite_guard's ``Side`` is built from"""
    gen = torch.Generator().manual_seed(0)
    base = [torch.randn(s, generator=gen) for s in SHAPES]
    grads = [torch.randn(s, generator=gen) * 3 for s in SHAPES]
    stats = torch.randn(65536 + 9, generator=gen)
    return base, grads, stats, None


def grad_buffers():
    return [device_grad(torch.zeros(s), i == MISALIGNED) for i, s in enumerate(SHAPES)]


def test_window_then_fused_step_equals_the_step_on_torch_accumulated_gradients(guard_data, sets):
    """two groups (one amsgrad, one maximize with its own lr), the clip at 5.0, an attached ModelEMA"""
    from solver import GradAccumulator
    A, B = Side(guard_data, guard=False), Side(guard_data, guard=False)
    # A: the window through the kernels, on the optimizer's own handle
    G = grad_buffers()
    for p, g in zip(A.net.w, G):
        p.grad = g
    acc = GradAccumulator(list(A.net.w), steps=2, engine=A.opt._engine)
    torch._foreach_copy_(G, sets[0])
    assert acc.accumulate() is False and acc.pending == 1
    torch._foreach_copy_(G, sets[1])
    versions = [g._version for g in G]
    assert acc.accumulate() is True and acc.pending == 0
    assert [g._version for g in G] == [v + 1 for v in versions]
    A.step(G, 1.0)
    # B: torch accumulates and scales
    B.step([device_grad((x + y) * 0.5, i == MISALIGNED) for i, (x, y) in enumerate(zip(sets[0], sets[1]))], 1.0)
    torch.cuda.synchronize()
    assert float(A.opt.last_grad_norm) > 5.0                        # the clip was active
    assert_same_bits(A.buffers(), B.buffers())                      # parameters, moments, averages, last_grad_norm


# ------------------------------------------------------------------------------------------------ 4. the guard
def test_a_nan_in_one_micro_batch_poisons_the_mean_and_the_guarded_step_is_skipped(guard_data, sets):
    from solver import GradAccumulator
    s = Side(guard_data, guard=True)
    G = grad_buffers()
    for p, g in zip(s.net.w, G):
        p.grad = g
    s.step(G, 1.0)                                                  # a first, taken step (zero gradients): the state exists
    before = {k: v.clone() for k, v in s.buffers().items() if k != "out_norm"}
    acc = GradAccumulator(list(s.net.w), steps=2, engine=s.opt._engine)
    i, off, _ = PLACES["second_chunk"]
    first = [g.clone() for g in sets[0]]
    first[i].view(-1)[off] = math.nan                               # in the FIRST micro-batch's gradient
    torch._foreach_copy_(G, first)
    assert acc.accumulate() is False
    torch._foreach_copy_(G, sets[1])
    assert acc.accumulate() is True
    torch.cuda.synchronize()
    mean = G[i].view(-1)
    assert math.isnan(float(mean[off])) and int(torch.isnan(mean).sum()) == 1
    assert all(bool(torch.isfinite(g).all()) for j, g in enumerate(G) if j != i)
    s.step(G, 1.0)
    recs = s.opt.drain_guard_reports(keep=0)
    assert [r.skipped for r in recs] == [False, True]
    assert recs[1].param is s.net.w[i] and recs[1].n_elements == 1 and math.isnan(recs[1].norm)
    after = {k: v for k, v in s.buffers().items() if k != "out_norm"}
    assert_same_bits(after, before)                                 # parameters, moments and averages keep every bit


# ------------------------------------------------------------------------------------------------ 5. arguments and state
class RawAccum:
    def __init__(self):
        from hipmonocon.engine import Engine
        gen = torch.Generator().manual_seed(9)
        self.eng = Engine(0)
        shapes = [(65536 + 5,), (131,), (16, 8)]
        self.n = len(shapes)
        self.g = [torch.randn(s, generator=gen).cuda() for s in shapes]
        self.a = [torch.randn(s, generator=gen).cuda() for s in shapes]
        self.numel = [t.numel() for t in self.g]

    def bind(self, g=None, a=None, numel=None, n=None):
        g, a = self.g if g is None else g, self.a if a is None else a
        numel = self.numel if numel is None else numel
        arr = (C.c_int64 * max(len(numel), 1))(*numel)
        return self.eng.lib.mc_accum_bind(self.eng.h, self.n if n is None else n, ptr_array(g), ptr_array(a), arr)

    def run(self, mode, scale=0.5):
        return self.eng.lib.mc_grad_accumulate(self.eng.h, mode, scale, stream())

    def err(self):
        return self.eng.lib.mc_last_error(self.eng.h).decode()

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in self.g + self.a]

    def unchanged(self, snap):
        torch.cuda.synchronize()
        return all(bits_equal(x, y) for x, y in zip(self.g + self.a, snap))


def test_argument_and_state_checks_fail_before_anything_is_launched():
    from hipmonocon.lib import ACCUM_ADD, ACCUM_BEGIN, ACCUM_FINISH
    r = RawAccum()
    start = r.snapshot()
    for mode in (ACCUM_BEGIN, ACCUM_ADD, ACCUM_FINISH):                      # no table bound
        assert r.run(mode) != 0 and "mc_accum_bind" in r.err(), mode
    for n in (0, -1):
        assert r.bind(n=n) != 0 and "bad argument" in r.err(), n
    assert r.bind(g=[r.g[0], None, r.g[2]]) != 0 and "null" in r.err()
    assert r.bind(a=[r.a[0], r.a[1], None]) != 0 and "null" in r.err()
    for bad in (0, -3):
        assert r.bind(numel=[r.numel[0], bad, r.numel[2]]) != 0 and "empty" in r.err(), bad
    assert r.bind(a=[r.a[0], r.g[1], r.a[2]]) != 0 and "alias" in r.err()           # an accumulator that is its gradient
    assert r.bind(a=[r.a[0], r.a[1], r.g[2].view(-1)[2:]], numel=[r.numel[0], r.numel[1], 100]) != 0 and "alias" in r.err()
    assert r.run(ACCUM_BEGIN) != 0 and "mc_accum_bind" in r.err()                   # a failed bind leaves nothing bound
    assert r.unchanged(start)
    assert r.bind() == 0, r.err()
    assert r.run(ACCUM_ADD) != 0 and "open window" in r.err()                       # ADD and FINISH without BEGIN
    assert r.run(ACCUM_FINISH) != 0 and "open window" in r.err()
    assert r.unchanged(start)
    assert r.run(ACCUM_BEGIN) == 0, r.err()
    opened = r.snapshot()
    assert all(bits_equal(a, g) for a, g in zip(r.a, r.g))                          # acc = g
    for mode in (3, -1, 17):
        assert r.run(mode) != 0 and "unknown mode" in r.err(), mode
    for bad in (math.nan, math.inf, -math.inf, 0.0, -0.5, 1e-60, 1e60):             # (the last two are no float32 > 0 / finite)
        assert r.run(ACCUM_FINISH, bad) != 0 and "scale" in r.err(), bad
    assert r.run(ACCUM_ADD, math.nan) == 0, r.err()                                 # ADD ignores scale; the window is still open
    added = r.snapshot()
    assert all(bits_equal(a, g + g) for a, g in zip(r.a, r.g))
    assert r.bind() == 0                                                            # a re-bind closes the window
    assert r.run(ACCUM_FINISH) != 0 and "open window" in r.err()
    assert r.run(ACCUM_ADD) != 0 and "open window" in r.err()
    assert r.unchanged(added)
    # BEGIN on an open window restarts it; FINISH closes it
    assert r.run(ACCUM_BEGIN, -1.0) == 0 and r.run(ACCUM_BEGIN, math.nan) == 0      # BEGIN ignores scale
    assert r.run(ACCUM_FINISH, 0.25) == 0, r.err()
    torch.cuda.synchronize()
    assert all(bits_equal(g, (s + s) * 0.25) for g, s in zip(r.g, opened[:r.n]))
    assert all(bits_equal(a, s) for a, s in zip(r.a, opened[:r.n]))                 # FINISH does not write acc
    done = r.snapshot()
    assert r.run(ACCUM_ADD) != 0 and r.run(ACCUM_FINISH) != 0 and "open window" in r.err()
    assert r.unchanged(done)


def test_accumulator_raises_on_a_gradient_that_moved_inside_a_window(sets):
    from hipmonocon.engine import Engine
    from hipmonocon.lib import MonoconHipError
    from solver import GradAccumulator
    params = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in BIG]
    for p, g in zip(params, sets[0]):
        p.grad = g.clone()
    acc = GradAccumulator(params, steps=3, engine=Engine(0))
    assert acc.accumulate() is False
    assert all(o % 4 == 0 for o in acc.offsets) and all(a.data_ptr() % 16 == 0 for a in acc.slices)
    params[1].grad = params[1].grad.clone()                         # what torch's own accumulation path would do
    snap = [p.grad.clone() for p in params] + [acc.flat.clone()]
    with pytest.raises(MonoconHipError, match="inside an open window"):
        acc.accumulate()
    torch.cuda.synchronize()
    assert acc.pending == 1 and all(bits_equal(x, y) for x, y in zip([p.grad for p in params] + [acc.flat], snap))
    # CPU gradients are refused by the binding: there is no torch fall-back
    cpu = [torch.nn.Parameter(torch.zeros(3))]
    cpu[0].grad = torch.ones(3)
    with pytest.raises(MonoconHipError):
        GradAccumulator(cpu, steps=2, engine=acc._engine).accumulate()


# ------------------------------------------------------------------------------------------------ 6, 7. the detector's step
BATCH_SEEDS = (GOLDEN_SEED + 41, GOLDEN_SEED + 42, GOLDEN_SEED + 43)


@pytest.fixture(scope="module")
def batches():
    return [to_cuda(synth.make_batch(seed, 2, 64, 128)) for seed in BATCH_SEEDS]


@pytest.fixture(scope="module")
def plain_steps(golden_sd, batches):
    """model A: one plain step per batch from the golden state (no optimizer in between); per step the ten losses and the
    flat gradient buffer"""
    m = build(golden_sd)
    out = []
    for b in batches:
        loss, _ = step(m, b)
        out.append((loss, m._train_binding.flat.flat.clone()))
    return out


def micro_batch(m, batch):
    for p in m.parameters():
        p.grad = None                                               # zero_grad(): set to none
    _, loss = m(batch)
    sum(loss.values()).backward()
    return torch.stack([v.detach() for v in loss.values()])


def test_detector_window_of_two_is_the_torch_mean_of_two_plain_steps(golden_sd, batches, plain_steps):
    from solver import GradAccumulator
    m = build(golden_sd)
    acc = GradAccumulator(m.parameters(), steps=2)
    ptrs = None
    for j in range(2):
        loss = micro_batch(m, batches[j])
        assert torch.equal(loss, plain_steps[j][0]), j
        here = [p.grad.data_ptr() for p in m.parameters() if p.grad is not None]
        assert ptrs is None or here == ptrs                         # no p.grad left the flat buffer: nothing was cloned
        ptrs = here
        assert acc.accumulate() is (j == 1)
    torch.cuda.synchronize()
    tb = m._train_binding
    assert ptrs == [tb.grads[n].data_ptr() for n, p in tb.named if p.grad is not None] and len(ptrs) == len(tb.grads)
    assert [p.grad.data_ptr() for p in m.parameters() if p.grad is not None] == ptrs
    assert torch.equal(tb.flat.flat, (plain_steps[0][1] + plain_steps[1][1]) * 0.5)
    assert len(acc.slices) == len(tb.grads)


def test_deferred_exchange_runs_once_per_window_on_a_world1_communicator(golden_sd, batches, plain_steps):
    from hipmonocon import train as htrain
    from solver import GradAccumulator
    m = build(golden_sd)
    eng = m._engine()                                               # the handle, before any step: the window below is steps 1..3
    assert hdist.ensure_engine_comm(eng, force=True)                # of this model, as plain_steps' are of its model
    try:
        was = eng.comm_info()["overlap"]
        assert was is True
        htrain.defer_grad_exchange(m, True)
        assert eng.comm_info()["overlap"] is False
        n0 = eng.comm_info()["launches"]
        acc = GradAccumulator(m.parameters(), steps=3)
        for j in range(3):
            loss = micro_batch(m, batches[j])
            assert torch.equal(loss, plain_steps[j][0]), j
            assert acc.accumulate() is (j == 2)
        assert eng.comm_info()["launches"] == n0                    # three backwards, no exchange
        htrain.exchange_grads_now(m)
        torch.cuda.synchronize()
        per = eng.comm_info()["collectives_per_exchange"]
        assert per > 0 and eng.comm_info()["launches"] == n0 + per  # one exchange for the window, not three
        third = f32(1.0 / 3.0)
        ref = (plain_steps[0][1] + plain_steps[1][1] + plain_steps[2][1]) * third
        assert torch.equal(m._train_binding.flat.flat, ref)         # an exchange over one rank is the identity
        htrain.defer_grad_exchange(m, False)
        assert eng.comm_info()["overlap"] is was
    finally:
        eng.comm_destroy()


# ------------------------------------------------------------------------------------------------ 8. the engine
def accum_cfg(out_dir):
    from utils.engine_utils import get_default_cfg
    cfg = get_default_cfg()
    cfg.set_new_allowed(True)
    cfg.OUTPUT_DIR = str(out_dir)
    cfg.SEED = 3
    cfg.DATA.ROOT = 'synthetic'
    cfg.DATA.SYNTHETIC_LENGTH = 10
    cfg.DATA.SYNTHETIC_HW = [96, 224]
    cfg.DATA.BATCH_SIZE = 2
    cfg.DATA.NUM_WORKERS = 0
    cfg.MODEL.BACKBONE.IMAGENET_PRETRAINED = False
    cfg.SOLVER.OPTIM.NUM_EPOCHS = 2
    cfg.SOLVER.ACCUM_STEPS = 2
    cfg.SOLVER.NONFINITE_GUARD.ENABLE = True
    cfg.SOLVER.EMA.ENABLE = True
    cfg.PERIOD.EVAL_PERIOD = 0
    cfg.PERIOD.LOG_PERIOD = 1
    return cfg


def test_engine_steps_once_per_window_and_closes_the_tail_window(tmp_path):
    from engine.monocon_engine import MonoconEngine
    from solver import GradAccumulator
    from utils.engine_utils import reduce_loss_dict, set_random_seed
    set_random_seed(3)
    eng = MonoconEngine(accum_cfg(tmp_path))
    assert len(eng.train_loader) == 5 and isinstance(eng.grad_accum, GradAccumulator) and eng.grad_accum.steps == 2
    assert eng.scheduler.total_steps == 3 * 2                       # ceil(5 / 2) optimizer steps an epoch, two epochs
    micro, ready, reports = [], [], []
    eng.model.register_forward_hook(lambda mod, args, out: micro.append(reduce_loss_dict(out[1]).detach().clone()))
    accumulate, account = eng.grad_accum.accumulate, eng.account_steps

    def spy_accumulate(last=False):
        ready.append(accumulate(last=last))
        return ready[-1]

    def spy_account(iters, losses, recs):
        reports.extend(recs)
        return account(iters, losses, recs)

    eng.grad_accum.accumulate, eng.account_steps = spy_accumulate, spy_account
    eng.train_one_epoch()
    torch.cuda.synchronize()
    assert ready == [False, True, False, True, True]                # windows of 2, 2 and the tail's 1
    assert eng.grad_accum.pending == 0 and len(micro) == 5
    assert eng.global_iters == 1 + 3 and eng.scheduler.last_epoch == 3 and eng.ema.updates == 3
    stepped = [p for p in eng.model.parameters() if p.grad is not None]
    assert stepped and all(int(eng.optimizer.state[p]['step']) == 3 for p in stepped)
    assert len(eng.optimizer.state) == len(stepped)
    want = [float(torch.stack(micro[0:2]).mean()), float(torch.stack(micro[2:4]).mean()), float(micro[4])]
    assert eng.entire_losses == want                                # one loss per window: the mean of its micro-batches
    assert len(reports) == 3 and [r.step for r in reports] == [1, 2, 3] and not any(r.skipped for r in reports)
    assert eng.skipped_steps == 0
    # BatchNorm's running statistics tick once per micro-batch, as in torch
    ticks = {int(v) for k, v in eng.model.state_dict().items() if k.endswith("num_batches_tracked")}
    assert ticks == {5}
