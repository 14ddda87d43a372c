"""The non-finite guard without a device: the SOLVER.NONFINITE_GUARD keys, the constructor's checks, the report queue of
``solver.fused_adamw`` against a stub library (order, ``keep``, no unbounded growth), and the engine's bookkeeping of skipped
steps (loss exclusion, the consecutive-skip limit, the buffer check) against a stub optimizer."""
import ctypes as C
import inspect
import math

import pytest
import torch


def test_config_defaults():
    from utils.engine_utils import get_default_cfg
    c = get_default_cfg()
    assert c.SOLVER.NONFINITE_GUARD.ENABLE is False and c.SOLVER.NONFINITE_GUARD.MAX_CONSECUTIVE == 10
    assert set(c.SOLVER.NONFINITE_GUARD.keys()) == {"ENABLE", "MAX_CONSECUTIVE"}


def test_constructor_validation_and_defaults():
    from solver import AdamW, clip_grad_norm_
    p = [torch.nn.Parameter(torch.zeros(3))]
    opt = AdamW(p)
    assert opt.skip_nonfinite is False and opt.skipped_steps == 0 and opt.drain_guard_reports(keep=0) == []
    assert AdamW(p, skip_nonfinite=True).skip_nonfinite is True
    assert AdamW(p, skip_nonfinite=True).skipped_steps == 0
    for bad in (1, 0, "yes", None):
        with pytest.raises(TypeError, match="skip_nonfinite"):
            AdamW(p, skip_nonfinite=bad)
    assert inspect.signature(AdamW.__init__).parameters["skip_nonfinite"].default is False
    assert inspect.signature(clip_grad_norm_).parameters["error_if_nonfinite"].default is False
    assert "skip_nonfinite" not in opt.state_dict()["param_groups"][0]       # torch's checkpoint layout is untouched


# ------------------------------------------------------------------------------------------------ the report queue
class Event:
    def __init__(self, fired):
        self.fired, self.waited = fired, False

    def query(self):
        return self.fired

    def synchronize(self):
        self.fired = self.waited = True


class StubLib:
    """``mc_optim_guard_report`` that writes the next scripted record straight into ``dst``"""

    def __init__(self, script, rc=0):
        self.script, self.calls, self.rc = list(script), 0, rc

    def mc_optim_guard_report(self, handle, dst, stream):
        if self.rc:
            return self.rc
        from hipmonocon.lib import GuardReport
        r = GuardReport.from_address(dst.value)
        r.skipped, r.first_tensor, r.n_elements, r.norm = self.script[self.calls]
        self.calls += 1
        return 0

    def mc_last_error(self, handle):
        return b"stub failure"


def make_queue(script, fired=True, max_pending=64):
    from hipmonocon.lib import GuardReport
    from solver.fused_adamw import GuardReportQueue
    slots, events = [], []

    def alloc():
        r = GuardReport()
        slots.append(r)
        return r, C.addressof(r)

    def event():
        events.append(Event(fired))
        return events[-1]

    return GuardReportQueue(alloc=alloc, event=event, max_pending=max_pending), StubLib(script), slots, events


PARAMS = ["p0", "p1", "p2"]
SCRIPT = [(0, -1, 0, 1.5), (1, 2, 4, math.inf), (0, -1, 0, 2.5), (1, -1, 0, math.inf), (1, 0, 1, math.nan)]


def push_all(q, lib, n=len(SCRIPT)):
    for k in range(n):
        q.push(lib, None, None, k + 1, PARAMS)


def test_queue_preserves_order_and_honours_keep():
    q, lib, slots, events = make_queue(SCRIPT, fired=False)
    push_all(q, lib, 3)
    assert q.skipped == 0                                       # nothing has landed: nothing is known, nothing is waited for
    assert q.ready(keep=3) == [] and q.ready(keep=7) == []
    got = q.ready(keep=1)
    assert [(r.step, r.skipped, r.param, r.n_elements, r.norm) for r in got] == [(1, False, None, 0, 1.5), (2, True, "p2", 4, math.inf)]
    assert [e.waited for e in events] == [True, True, False]    # only what was returned was waited for
    assert len(q.pending) == 1 and q.skipped == 1
    push_all_from = 3
    for k in range(push_all_from, 5):
        q.push(lib, None, None, k + 1, PARAMS)
    assert len(slots) == 3                                      # the slots of the two records read are used again
    events[2].fired = events[3].fired = True
    assert q.skipped == 2                                       # step 4 has landed and is counted, step 5 is still in flight
    got = q.ready(keep=0)
    assert [r.step for r in got] == [3, 4, 5] and [r.skipped for r in got] == [False, True, True]
    assert got[1].param is None and got[1].n_elements == 0      # an overflowed norm: no culprit
    assert got[2].param == "p0" and math.isnan(got[2].norm)
    assert q.skipped == 3 and not q.pending and q.ready(keep=0) == []


def test_queue_does_not_grow_in_a_loop_that_never_reads():
    script = [(k % 3 == 0, 1 if k % 3 == 0 else -1, k % 3 == 0, 1.0) for k in range(200)]
    q, lib, slots, events = make_queue(script, fired=True, max_pending=8)
    push_all(q, lib, 200)
    assert len(q.pending) == 8 and len(slots) <= 9
    assert q.skipped == sum(1 for s in script if s[0])          # the dropped entries were counted
    assert [r.step for r in q.ready(keep=0)] == list(range(193, 201))
    # entries whose copy has not landed are never dropped: they are not known yet
    q, lib, slots, events = make_queue(script, fired=False, max_pending=8)
    push_all(q, lib, 20)
    assert len(q.pending) == 20 and q.skipped == 0
    for e in events[:15]:
        e.fired = True
    q.push(lib, None, None, 21, PARAMS)
    assert len(q.pending) == 8 and [e[0] for e in q.pending] == list(range(14, 22))


def test_queue_reports_a_failed_call(monkeypatch):
    import hipmonocon.lib as L
    q, _, _, _ = make_queue(SCRIPT)
    lib = StubLib(SCRIPT, rc=-1)
    monkeypatch.setattr(L, "load", lambda: lib)                 # check() asks the library for the handle's message
    with pytest.raises(L.MonoconHipError, match="mc_optim_guard_report.*stub failure"):
        q.push(lib, None, None, 1, PARAMS)
    assert not q.pending


# ------------------------------------------------------------------------------------------------ the engine's bookkeeping
class StubOptimizer:
    """what the loop sees of the fused AdamW: ``skip_nonfinite`` and ``drain_guard_reports``"""
    skip_nonfinite = True

    def __init__(self, records):
        self.records = list(records)

    def drain_guard_reports(self, keep=1):
        n = max(len(self.records) - keep, 0)
        out, self.records = self.records[:n], self.records[n:]
        return out


def stub_engine(max_consecutive=3):
    from engine.monocon_engine import MonoconEngine
    eng = object.__new__(MonoconEngine)
    eng.rank, eng.weight_dir = 0, "/somewhere/checkpoints"
    eng.model = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
    eng.skipped_steps, eng.consecutive_skips, eng.max_consecutive_skips = 0, 0, max_consecutive
    return eng


def rec(step, skipped, param=None, n=0, norm=1.0):
    from solver.fused_adamw import GuardRecord
    return GuardRecord(step, skipped, param, n, norm)


def test_engine_excludes_the_loss_of_a_skipped_step_and_names_the_parameter(capsys):
    eng = stub_engine()
    w = eng.model[0].bias
    opt = StubOptimizer([rec(1, False), rec(2, True, w, 3, math.inf), rec(3, False), rec(4, True, None, 0, math.inf), rec(5, False)])
    reports = opt.drain_guard_reports(keep=1)
    assert len(reports) == 4
    taken = eng.account_steps([11, 12, 13, 14], [1.0, math.nan, 3.0, 4.0], reports)
    assert taken == [1.0, 3.0]
    assert eng.skipped_steps == 2 and eng.consecutive_skips == 1
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if "SKIPPED" in l]
    assert len(lines) == 2
    assert "Iteration 12:" in lines[0] and "'0.bias'" in lines[0] and "3 non-finite element" in lines[0] and "inf" in lines[0]
    assert "Iteration 14:" in lines[1] and "overflowed" in lines[1] and "2 step(s) skipped so far" in lines[1]
    assert eng.account_steps([15], [5.0], opt.drain_guard_reports(keep=0)) == [5.0]
    assert eng.consecutive_skips == 0 and eng.skipped_steps == 2
    # steps that were not guarded at all pass through
    assert eng.account_steps([16, 17], [6.0, 7.0], [None, None]) == [6.0, 7.0]


def test_engine_raises_after_max_consecutive_skips_and_not_before():
    eng = stub_engine(max_consecutive=3)
    w = eng.model[0].weight
    skip = lambda k: rec(k, True, w, 1, math.nan)      # noqa: E731
    assert eng.account_steps([1, 2, 3, 4, 5], [0.0] * 5, [skip(1), skip(2), rec(3, False), skip(4), skip(5)]) == [0.0]
    assert eng.consecutive_skips == 2 and eng.skipped_steps == 4
    with pytest.raises(RuntimeError, match=r"3 optimizer steps in a row .*MAX_CONSECUTIVE.*/somewhere/checkpoints"):
        eng.account_steps([6, 7], [0.0, 0.0], [skip(6), rec(7, False)])
    assert eng.skipped_steps == 5


def test_engine_raises_when_the_forward_pass_poisoned_the_buffers():
    eng = stub_engine()
    with torch.no_grad():
        eng.model[1].running_var[2] = math.nan
    with pytest.raises(RuntimeError, match=r"'1.running_var'.*last checkpoint in '/somewhere/checkpoints'"):
        eng.account_steps([9], [math.nan], [rec(1, True, eng.model[0].weight, 7, math.nan)])
    assert eng.skipped_steps == 1
    # a taken step does not look at the buffers: that check is the rare path's
    assert eng.account_steps([10], [1.0], [rec(2, False)]) == [1.0]


def test_skipped_steps_travels_in_the_engine_attributes():
    from engine.base_engine import BaseEngine
    for k in ("consecutive_skips", "max_consecutive_skips"):
        assert k in BaseEngine._ATTR_EXCEPT                      # the run's own, never taken from a file
    assert "skipped_steps" not in BaseEngine._ATTR_EXCEPT
