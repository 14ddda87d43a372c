"""Gradient accumulation without a device: the launches ``solver.GradAccumulator`` asks of its engine for every window
length (against a recording engine; the object takes ``engine=`` as ``GuardReportQueue`` takes ``alloc`` / ``event``), the
layout of its flat accumulator, the constructor's checks, the schedule length of the engine and the config default."""
import math

import pytest
import torch


class RecordingEngine:
    """what the accumulator needs of ``hipmonocon.engine.Engine``: ``accum_bind`` and ``grad_accumulate``, recorded"""

    def __init__(self):
        self.binds, self.calls = [], []

    def accum_bind(self, grads, accs):
        self.binds.append(([g.data_ptr() for g in grads], [a.data_ptr() for a in accs], [g.numel() for g in grads]))

    def grad_accumulate(self, mode, scale=1.0):
        self.calls.append((mode, scale))


SHAPES = [(3, 5), (1,), (131,), (8,), (6,)]
NO_GRAD = 3


def make_params():
    gen = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in SHAPES]
    for i, p in enumerate(params):
        if i != NO_GRAD:
            p.grad = torch.randn(p.shape, generator=gen)
    return params


def expected(k):
    """the issue's sequence for a window of k micro-batches"""
    from hipmonocon.lib import ACCUM_ADD, ACCUM_BEGIN, ACCUM_FINISH
    if k == 1:
        return []
    return [ACCUM_BEGIN] + [ACCUM_ADD] * (k - 2) + [ACCUM_FINISH]


def check_calls(calls, k):
    from hipmonocon.lib import ACCUM_FINISH
    assert [m for m, _ in calls] == expected(k), (k, calls)
    for m, s in calls:
        if m == ACCUM_FINISH:
            assert s == 1.0 / k             # folded in double, exactly


@pytest.mark.parametrize("steps", (1, 2, 3, 4))
def test_mode_and_scale_sequence_of_full_windows(steps):
    from solver import GradAccumulator
    eng = RecordingEngine()
    acc = GradAccumulator(make_params(), steps=steps, engine=eng)
    for window in range(3):
        eng.calls.clear()
        for i in range(steps):
            assert acc.pending == i
            ready = acc.accumulate()
            assert ready is (i == steps - 1)
        assert acc.pending == 0
        check_calls(eng.calls, steps)
    assert len(eng.binds) == (0 if steps == 1 else 1)           # bound once: no gradient moved


@pytest.mark.parametrize("steps,tail", ((4, 1), (4, 2), (4, 3), (3, 2), (2, 1)))
def test_a_tail_window_closes_with_its_own_count(steps, tail):
    from solver import GradAccumulator
    eng = RecordingEngine()
    acc = GradAccumulator(make_params(), steps=steps, engine=eng)
    for i in range(tail):
        assert acc.accumulate(last=(i == tail - 1)) is (i == tail - 1)
    check_calls(eng.calls, tail)
    assert acc.pending == 0 and acc.flush() is False
    eng.calls.clear()                                           # and the next epoch starts a full window
    for i in range(steps):
        acc.accumulate()
    check_calls(eng.calls, steps)


def test_window_modes_helper_is_the_same_sequence():
    from solver.grad_accum import window_modes
    for k in (1, 2, 3, 4, 7):
        modes = window_modes(k)
        assert [m for m, _ in modes] == expected(k)
        if k > 1:
            assert modes[-1][1] == 1.0 / k and all(s is None for _, s in modes[:-1])


def test_flush_is_false_when_idle_and_an_error_on_an_open_window():
    from hipmonocon.lib import MonoconHipError
    from solver import GradAccumulator
    acc = GradAccumulator(make_params(), steps=3, engine=RecordingEngine())
    assert acc.flush() is False
    assert acc.accumulate() is False
    with pytest.raises(MonoconHipError, match=r"last=True"):
        acc.flush()
    assert acc.pending == 1                                     # nothing was dropped


def test_table_is_the_parameters_with_a_gradient_in_order_and_slices_start_at_multiples_of_four():
    from solver import GradAccumulator
    eng = RecordingEngine()
    params = make_params()
    acc = GradAccumulator(params, steps=2, engine=eng)
    acc.accumulate()
    with_grad = [p for i, p in enumerate(params) if i != NO_GRAD]
    gptr, aptr, numel = eng.binds[0]
    assert gptr == [p.grad.data_ptr() for p in with_grad] and numel == [p.numel() for p in with_grad]
    assert acc.offsets == [0, 16, 20, 152] and all(o % 4 == 0 for o in acc.offsets)
    assert acc.flat.numel() == 160 and acc.flat.dtype == torch.float32
    assert aptr == [acc.flat.data_ptr() + 4 * o for o in acc.offsets]
    assert [s.numel() for s in acc.slices] == numel


def test_rebinds_only_when_a_gradient_moved_and_raises_inside_a_window():
    from hipmonocon.lib import MonoconHipError
    from solver import GradAccumulator
    eng = RecordingEngine()
    params = make_params()
    acc = GradAccumulator(params, steps=3, engine=eng)
    for _ in range(6):
        acc.accumulate()
    assert len(eng.binds) == 1
    params[0].grad = params[0].grad.clone()                     # between windows: bound again
    acc.accumulate()
    assert len(eng.binds) == 2 and acc.pending == 1
    params[2].grad = params[2].grad.clone()                     # inside the window: an error, nothing launched, nothing dropped
    n = len(eng.calls)
    with pytest.raises(MonoconHipError, match="inside an open window"):
        acc.accumulate()
    assert len(eng.calls) == n and len(eng.binds) == 2 and acc.pending == 1


def test_finish_advances_the_gradients_versions():
    from solver import GradAccumulator
    params = make_params()
    acc = GradAccumulator(params, steps=2, engine=RecordingEngine())
    before = [p.grad._version for p in params if p.grad is not None]
    acc.accumulate()
    assert [p.grad._version for p in params if p.grad is not None] == before
    acc.accumulate()
    assert [p.grad._version for p in params if p.grad is not None] == [v + 1 for v in before]


def test_steps_is_validated():
    from solver import GradAccumulator
    p = make_params()
    for bad in (0, -1, -7):
        with pytest.raises(ValueError, match="steps"):
            GradAccumulator(p, steps=bad)
    for bad in (2.0, 1.5, "2", None, True):
        with pytest.raises(TypeError, match="steps"):
            GradAccumulator(p, steps=bad)
    assert GradAccumulator(p, steps=1).steps == 1 and GradAccumulator(p, steps=8).steps == 8


@pytest.mark.parametrize("length,steps,epochs", ((8, 2, 3), (8, 4, 1), (5, 2, 3), (7, 3, 2), (3, 4, 5), (6, 1, 2), (1, 1, 1)))
def test_schedule_length_counts_optimizer_steps(length, steps, epochs):
    from solver.grad_accum import optimizer_steps_per_epoch
    assert optimizer_steps_per_epoch(length, steps) * epochs == math.ceil(length / steps) * epochs


def test_build_solver_sizes_the_schedule_by_optimizer_steps():
    """the engine's own build_solver on a stub: 5 batches in windows of 2 are 3 steps an epoch"""
    from engine.monocon_engine import MonoconEngine
    from utils.engine_utils import get_default_cfg
    for steps, want in ((1, 5 * 4), (2, 3 * 4), (5, 1 * 4), (8, 1 * 4)):
        cfg = get_default_cfg()
        cfg.SOLVER.ACCUM_STEPS = steps
        cfg.SOLVER.OPTIM.NUM_EPOCHS = 4
        eng = object.__new__(MonoconEngine)
        eng.cfg, eng.ema = cfg, None
        eng.model = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
        eng.train_loader = [None] * 5
        _, sched = eng.build_solver()
        assert sched.total_steps == want, (steps, sched.total_steps)
        assert (eng.grad_accum is None) == (steps == 1)
        if steps > 1:
            assert eng.grad_accum.steps == steps and eng.grad_accum.pending == 0


def test_config_default_and_checkpoint_attributes():
    from engine.base_engine import BaseEngine
    from utils.engine_utils import get_default_cfg
    assert get_default_cfg().SOLVER.ACCUM_STEPS == 1
    assert "grad_accum" in BaseEngine._ATTR_EXCEPT              # the run's own object, never pickled into a checkpoint
