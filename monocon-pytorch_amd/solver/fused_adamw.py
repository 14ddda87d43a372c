"""Fused gradient-clip + AdamW on MI355X.

Drop-in for ``torch.optim.AdamW`` in the reference train loop (engine/monocon_engine.py:35-55,
94-102).  The class is deliberately named ``AdamW`` (CyclicScheduler asserts on the class name,
solver/cyclic_scheduler.py:16-17).  ``step()`` launches libmonocon_hip's multi-tensor kernels:
global gradient norm (any ``norm_type`` of ``clip_grad_norm_``), clip coefficient and the
decoupled-weight-decay Adam update in two passes over the parameters instead of hundreds of
per-tensor launches.  Parameters without a gradient (the six tensors the reference never
back-propagates into, SURVEY §8a quirk i) are skipped, as torch does.

Any number of parameter groups, each with its own ``lr``, ``betas``, ``eps``, ``weight_decay``,
``amsgrad`` and ``maximize``, and a step count per parameter, as ``torch.optim.AdamW`` keeps them: the
distinct (hyper-parameters, step) sets of one ``step()`` -- its *classes* -- go to the kernel as a
table of at most ``MC_OPT_MAX_CLASSES`` rows, every bound tensor carries the index of its row.
``clip_grad_norm_`` is ``torch.nn.utils.clip_grad_norm_`` as three launches for the loop that clips
by itself.

``set_ema(ema)`` attaches a ``solver.ModelEMA``: the AdamW pass then also updates the average of every
parameter it steps, from the new value while it is in registers (``mc_optim_bind_ema`` +
``mc_clip_adamw_ema_step_classes``: 8 B/param more, no further launch), and ``step()`` ends with one
``mc_ema_update`` over the rest of the model's state (BatchNorm running statistics, parameters
without a gradient).  A loop with an attached average does not call ``ema.update`` itself.

``skip_nonfinite=True`` guards the step against a non-finite gradient (torch's fused AdamW has ``found_inf``, ``GradScaler``
skips the step): when the global norm, as computed, is NaN or infinite, the AdamW pass writes nothing -- parameters, moments,
``max_exp_avg_sq``, the attached averages and (``mc_ema_update_guarded``) the rest of the average keep every bit -- and
records which tensor held how many NaN/inf elements.  The decision is taken on the device from the norm that is already
there: no host round trip, no further launch.  A skipped step still COUNTS: ``state[p]['step']``, ``ModelEMA.updates`` and
a scheduler advance as for a taken one, because the step counts are folded into the kernel's arguments before the launch
and the host does not wait to learn the outcome; the report carries the skip, a caller who wants taken steps subtracts.
Every ``step()`` enqueues a copy of the device record into a page-locked slot behind an event; ``skipped_steps`` and
``drain_guard_reports(keep=1)`` read them without a synchronisation.  Under data parallelism every rank sees the same
all-reduced gradients, computes the same norm and takes the same decision: no collective is added.

``trust_ratio=True`` turns the step into LAMB (You et al. 2019; timm's ``Lamb``, apex's ``FusedLAMB``): the Adam update ``u`` of
every tensor -- weight decay included -- is rescaled by the tensor's trust ratio ``r = |p| / |u|`` before it is applied,
``p -= lr * r * u`` (``mc_clip_lamb_step_classes``, the formula in include/monocon_hip.h: three launches behind the global norm
instead of AdamW's one, 40 B/param instead of 16).  A group adapts when its ``trust_ratio`` is on (the constructor's value, or
the group's own key) and it has ``weight_decay > 0`` or ``always_adapt`` is set -- timm's convention, which leaves the biases
and norm weights of a no-decay group at ``r = 1``, AdamW up to rounding.  ``trust_clip > 0`` caps ``r``.  The state is AdamW's
(``step``, ``exp_avg``, ``exp_avg_sq``), so checkpoints move freely between the two modes; ``load_state_dict`` keeps this
optimizer's own ``trust_ratio`` settings.  ``amsgrad`` is not supported with it.  ``trust_ratios()`` reads the last step's
ratios for logging.  ``set_ema``, ``skip_nonfinite``, ``GradAccumulator`` and data parallelism work as before: every rank steps
on the same all-reduced gradients and forms the same norms and ratios from the same parameters, so no collective is added.
With every ``trust_ratio`` off, ``step()`` is the AdamW path above, call for call.
"""
import collections
import ctypes as C

import torch
from torch.optim.optimizer import Optimizer

from hipmonocon import lib as _lib

MAX_CLASSES = _lib.OPT_MAX_CLASSES
_TORCH_DEFAULTS = None


def _torch_defaults():
    """torch.optim.AdamW's own ``defaults`` (foreach, capturable, differentiable, fused, ...): carried in every group so that
    ``state_dict()`` has torch's keys; the fused step reads none of the extra ones"""
    global _TORCH_DEFAULTS
    if _TORCH_DEFAULTS is None:
        _TORCH_DEFAULTS = dict(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).defaults)
    return _TORCH_DEFAULTS


def check_norm_type(norm_type):
    p = float(norm_type)
    if not p > 0.0:                                  # p <= 0 and NaN
        raise ValueError("norm_type must be > 0 (inf allowed), got %r" % (norm_type,))
    return p


def class_key(group, step):
    """the tuple that makes two (group, step) pairs one class of the kernel's table"""
    b1, b2 = group['betas']
    return (float(group['lr']), float(b1), float(b2), float(group['eps']), float(group['weight_decay']), int(step),
            bool(group.get('amsgrad', False)), bool(group.get('maximize', False)))


def fold_classes(param_groups, pairs):
    """``pairs``: (group index, 1-based step) per bound tensor, in table order.  Returns (classes, cls): the distinct
    ``class_key`` tuples in order of first appearance and each tensor's index into them.  More than ``MAX_CLASSES``
    distinct classes raise."""
    index, classes, by_key = {}, [], {}
    for pair in dict.fromkeys(pairs):
        key = class_key(param_groups[pair[0]], pair[1])
        k = by_key.get(key)
        if k is None:
            k = by_key[key] = len(classes)
            classes.append(key)
            if k >= MAX_CLASSES:
                raise _lib.MonoconHipError(
                    "fused AdamW: this step needs more than %d hyper-parameter classes (distinct lr / betas / eps / "
                    "weight_decay / amsgrad / maximize of the groups times distinct step counts of their parameters)"
                    % MAX_CLASSES)
        index[pair] = k
    return classes, tuple(map(index.__getitem__, pairs))


def fold_lamb_classes(param_groups, pairs, adapts):
    """``fold_classes`` for a LAMB step: ``adapts[gi]`` tells whether group ``gi`` uses the trust ratio, and two pairs are one
    class when ``class_key(...) + (adapts,)`` agree.  Returns (classes, cls, adapt_mask): the ``class_key`` tuples in order of
    first appearance, each tensor's index into them, and bit c set when class c adapts."""
    index, classes, by_key, mask = {}, [], {}, 0
    for pair in dict.fromkeys(pairs):
        key = class_key(param_groups[pair[0]], pair[1]) + (bool(adapts[pair[0]]),)
        k = by_key.get(key)
        if k is None:
            k = by_key[key] = len(classes)
            classes.append(key[:-1])
            if k >= MAX_CLASSES:
                raise _lib.MonoconHipError(
                    "fused LAMB: this step needs more than %d hyper-parameter classes (distinct lr / betas / eps / weight_decay "
                    "/ maximize / adapting of the groups times distinct step counts of their parameters)" % MAX_CLASSES)
            mask |= int(key[-1]) << k
        index[pair] = k
    return classes, tuple(map(index.__getitem__, pairs)), mask


def check_trust_clip(trust_clip):
    c = float(trust_clip)
    if not 0.0 <= c < float("inf"):                  # negative, NaN and inf
        raise ValueError("trust_clip must be finite and >= 0 (0: no cap), got %r" % (trust_clip,))
    return c


def _check_tensor(t, like, what):
    if t.dtype != torch.float32 or t.device != like.device or not t.is_contiguous():
        raise _lib.MonoconHipError("fused AdamW: %s must be a contiguous float32 tensor on the parameter's device" % what)


GuardRecord = collections.namedtuple("GuardRecord", "step skipped param n_elements norm")
GuardRecord.__doc__ = """one guarded ``step()``: its 1-based index among this optimizer's ``step()`` calls, whether it was skipped,
the first bound parameter (table order: groups in order, parameters in order) with a NaN/inf gradient element (None: none --
a taken step, or a norm that overflowed from finite elements), the number of such elements, the norm as computed"""


def _pinned_slot():
    t = torch.empty(C.sizeof(_lib.GuardReport), dtype=torch.uint8, pin_memory=True)
    return t, t.data_ptr()


def _recorded_event():
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream())
    return ev


class GuardReportQueue:
    """The ``DeferredScalars`` pattern (hipmonocon/feed.py) for ``mc_guard_report`` records: ``push`` enqueues the copy of the
    handle's device record into a page-locked slot and an event behind it, ``ready(keep)`` returns, in order, the records of
    all but the ``keep`` newest steps (``keep=0``: all, a synchronisation on the newest), ``skipped`` counts what is known
    without waiting.  A loop that never reads does not grow the queue: beyond ``max_pending`` entries, the oldest whose event
    has fired are counted and dropped.  ``alloc`` (-> (owner, address)) and ``event`` (-> an object with ``query`` and
    ``synchronize``) default to page-locked memory and a recorded ``torch.cuda.Event``."""

    def __init__(self, alloc=None, event=None, max_pending=64):
        self._alloc, self._event, self.max_pending = alloc or _pinned_slot, event or _recorded_event, int(max_pending)
        self.pending = collections.deque()      # (step index, bound parameters, slot, event)
        self._free = []                         # slots of entries that were read
        self._skipped = 0                       # skipped steps among the entries that have left the queue

    def push(self, lib, handle, stream, step, params):
        slot = self._free.pop() if self._free else self._alloc()
        _lib.check(handle, lib.mc_optim_guard_report(handle, C.c_void_p(slot[1]), stream), "mc_optim_guard_report")
        self.pending.append((step, params, slot, self._event()))
        while len(self.pending) > self.max_pending and self.pending[0][3].query():
            self._pop()

    def _read(self, entry):
        step, params, slot, _ = entry
        r = _lib.GuardReport.from_address(slot[1])
        k = int(r.first_tensor)
        return GuardRecord(step, bool(r.skipped), params[k] if 0 <= k < len(params) else None, int(r.n_elements), float(r.norm))

    def _pop(self):
        entry = self.pending.popleft()
        rec = self._read(entry)
        self._free.append(entry[2])
        self._skipped += rec.skipped
        return rec

    def ready(self, keep=1):
        out = []
        while len(self.pending) > max(int(keep), 0):
            self.pending[0][3].synchronize()
            out.append(self._pop())
        return out

    @property
    def skipped(self):
        return self._skipped + sum(self._read(e).skipped for e in self.pending if e[3].query())


class AdamW(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False,
                 max_grad_norm=None, norm_type=2.0, engine=None, skip_nonfinite=False, trust_ratio=False, trust_clip=0.0,
                 always_adapt=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if not isinstance(skip_nonfinite, bool):
            raise TypeError("skip_nonfinite must be a bool, got %r" % (skip_nonfinite,))
        defaults = dict(_torch_defaults())
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
        # LAMB.  trust_ratio is no entry of `defaults`: the groups keep torch.optim.AdamW's keys, a group that sets its own
        # 'trust_ratio' carries that one key more.  (Set before the groups are added: add_param_group checks against them.)
        self.trust_ratio = bool(trust_ratio)
        self.trust_clip = check_trust_clip(trust_clip)
        self.always_adapt = bool(always_adapt)
        self._ratio_params = None       # the bound parameters of the last LAMB step (trust_ratios)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.norm_type = check_norm_type(norm_type)
        self._engine = engine
        self._ema = None                # solver.ModelEMA whose update step() performs (set_ema)
        self._bound_sig = None
        self._step_cache = None         # (key, host-side copies of the bound tensors' step counts); None: re-read the state
        self.last_grad_norm = None      # device scalar of the most recent pre-clip norm
        self.skip_nonfinite = skip_nonfinite
        self._step_calls = 0            # guarded step() calls so far: the step index of the guard's records
        self._guard_reports = GuardReportQueue() if skip_nonfinite else None

    def set_engine(self, engine):
        self._engine = engine
        self._bound_sig = None

    @property
    def skipped_steps(self):
        """skipped steps known so far (0 without ``skip_nonfinite``): every report whose copy has landed, no synchronisation"""
        return self._guard_reports.skipped if self._guard_reports is not None else 0

    def drain_guard_reports(self, keep=1):
        """``GuardRecord`` s, oldest first, of all guarded steps but the ``keep`` newest -- whose copies may still be in flight;
        ``keep=0`` returns all and synchronises on the newest.  Each record is returned once."""
        return self._guard_reports.ready(keep) if self._guard_reports is not None else []

    def set_ema(self, ema):
        """Attach (None: detach) a ``solver.ModelEMA``.  From now on ``step()`` performs the average's whole update: the
        stepped parameters inside the AdamW pass, the rest of the model's state with one ``mc_ema_update``, then
        ``ema.updates += 1``.  The caller must NOT call ``ema.update()`` as well -- that would average twice per step."""
        self._ema = ema
        self._bound_sig = None

    def load_state_dict(self, state_dict):
        """Restores the moments and the per-parameter ``step`` (torch.optim.AdamW's checkpoint layout, which
        is what the reference saves, engine/base_engine.py:155-219).  The kernels hold raw pointers to the moment
        tensors, which torch replaces here: the binding is dropped and rebuilt on the next step()."""
        own = [g.get('trust_ratio') for g in self.param_groups]
        super().load_state_dict(state_dict)
        # LAMB or not is this optimizer's choice, not the file's: the state is the same in both modes
        for g, t in zip(self.param_groups, own):
            g.pop('trust_ratio', None)
            if t is not None:
                g['trust_ratio'] = t
        self._bound_sig = None
        self._step_cache = None
        # torch hands the caller's own 'step' (and same-device moment) tensors through uncopied; step() updates
        # them in place, so take private copies -- loading one checkpoint dict into two optimizers stays safe
        for st in self.state.values():
            for key in ('step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'):
                if key in st and torch.is_tensor(st[key]):
                    st[key] = st[key].clone()

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for k, v in _torch_defaults().items():
                group.setdefault(k, v)
        self._bound_sig = None
        self._step_cache = None

    def add_param_group(self, param_group):
        # one launch steps every group, and the LAMB step has no amsgrad form: no amsgrad group beside a trust_ratio one
        if isinstance(param_group, dict):
            flags = [(bool(g.get('amsgrad', self.defaults['amsgrad'])), bool(g.get('trust_ratio', self.trust_ratio)))
                     for g in self.param_groups + [param_group]]
            if any(a for a, _ in flags) and any(t for _, t in flags):
                raise ValueError("amsgrad is not supported together with trust_ratio (LAMB)")
        super().add_param_group(param_group)
        self._bound_sig = None
        self._step_cache = None

    def _adapts(self):
        """per group: does it use the trust ratio (None: no group has ``trust_ratio`` on -- the AdamW path)"""
        on = [bool(g.get('trust_ratio', self.trust_ratio)) for g in self.param_groups]
        if not any(on):
            return None
        return [t and (float(g['weight_decay']) > 0.0 or self.always_adapt) for g, t in zip(self.param_groups, on)]

    def trust_ratios(self, adapting_only=False):
        """``{parameter: trust ratio}`` of the last LAMB ``step()`` (1.0 where the group does not adapt; ``adapting_only``
        leaves those out): one copy of n floats and a synchronisation, only when called -- for logging.  After a step the
        guard skipped: the ratios of the step before."""
        if self._ratio_params is None:
            raise _lib.MonoconHipError("trust_ratios: no step() with trust_ratio on has run")
        plist, eng = self._ratio_params, self._engine
        out = torch.empty(len(plist), dtype=torch.float32, device=plist[0].device)
        with torch.cuda.device(plist[0].device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(eng.h, eng.lib.mc_lamb_ratios(eng.h, C.c_void_p(out.data_ptr()), len(plist), stream), "mc_lamb_ratios")
        ratios = dict(zip(plist, out.cpu().tolist()))
        if adapting_only:
            keep = {p for g, a in zip(self.param_groups, self._adapts() or ()) if a for p in g['params']}
            ratios = {p: r for p, r in ratios.items() if p in keep}
        return ratios

    def zero_state(self):
        """forget the moments and step counts (a fresh optimizer over the same parameters)"""
        self.state.clear()
        self._bound_sig = None
        self._step_cache = None

    def _init_state(self, p, amsgrad):
        """torch.optim.AdamW's lazy state of one parameter"""
        st = self.state[p]
        if len(st) == 0:
            st['step'] = torch.tensor(0.0)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if amsgrad and 'max_exp_avg_sq' not in st:
            st['max_exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _steps(self, plist, states):
        """The bias-correction step lives in ``state[p]['step']`` only (so it survives state_dict round trips).  Reading
        it back is one ``int()`` per tensor -- a host sync each if a resumed checkpoint left the step tensors on the
        device -- so the counts are read once (after construction / load_state_dict / a change of the parameter list) and
        tracked on the host, one per tensor, from then on."""
        # keyed on the IDENTITY of the stepped tensors and of their step objects (the length alone let a changed
        # parameter set of equal size, a reset state or a user-edited state[p]['step'] reuse a stale host copy)
        key = tuple([(id(p), id(st['step'])) for p, st in zip(plist, states)])
        if self._step_cache is None or self._step_cache[0] != key:
            self._step_cache = (key, [int(st['step']) for st in states])
        return self._step_cache[1]

    def _bind(self, plist, states, ams, cls, emas=None):
        eng = self._engine
        if eng is None:
            from hipmonocon.engine import Engine
            eng = self._engine = Engine(plist[0].device.index)
        # re-bound only when a pointer or a class index changes: lr moves every step, the class assignment does not
        # (the averages of an attached ModelEMA are part of the same signature: one cache for both bindings)
        sig = (tuple([(p.data_ptr(), p.grad.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(),
                       st['max_exp_avg_sq'].data_ptr() if a else 0) for p, st, a in zip(plist, states, ams)]), cls,
               None if emas is None else tuple([0 if e is None else e.data_ptr() for e in emas]))
        if sig == self._bound_sig and getattr(eng, '_optim_sig', None) is self._bound_sig:
            return eng
        n = len(plist)
        P, G, M, V, X = ((C.c_void_p * n)() for _ in range(5))
        N = (C.c_int64 * n)()
        K = (C.c_int * n)(*cls)
        for i, (p, st, a) in enumerate(zip(plist, states, ams)):
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or not p.grad.is_contiguous() or \
                    p.grad.dtype != torch.float32 or p.grad.device != p.device:
                raise _lib.MonoconHipError("fused AdamW needs contiguous float32 HIP parameters and gradients")
            for key in ('exp_avg', 'exp_avg_sq') + (('max_exp_avg_sq',) if a else ()):
                _check_tensor(st[key], p, "state['%s']" % key)
            P[i], G[i], M[i], V[i], X[i] = sig[0][i]
            N[i] = p.numel()
            if emas is not None and emas[i] is not None:
                _check_tensor(emas[i], p, "the ModelEMA tensor of a stepped parameter")
                if emas[i].numel() != p.numel():
                    raise _lib.MonoconHipError("fused AdamW: a ModelEMA tensor and its parameter differ in size")
        _lib.check(eng.h, eng.lib.mc_optim_bind_classes(eng.h, n, P, G, M, V, X, N, K), "mc_optim_bind_classes")
        if emas is not None:
            E = (C.c_void_p * n)(*[e or None for e in sig[2]])
            _lib.check(eng.h, eng.lib.mc_optim_bind_ema(eng.h, n, E), "mc_optim_bind_ema")
        self._bound_sig = eng._optim_sig = sig
        return eng

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # the bound table: the groups in order, each in parameter order, restricted to parameters with a gradient
        plist, gis, ams = [], [], []
        for gi, group in enumerate(self.param_groups):
            a = bool(group.get('amsgrad', False))
            for p in group['params']:
                if p.grad is not None:
                    plist.append(p)
                    gis.append(gi)
                    ams.append(a)
        if not plist:
            if self._ema is not None:           # nothing to step: the average still follows the buffers
                self._ema.update()
            return loss
        states = [self._init_state(p, a) for p, a in zip(plist, ams)]
        steps = self._steps(plist, states)
        for i in range(len(steps)):
            steps[i] += 1
        ema = self._ema
        adapts = self._adapts()                 # None: AdamW
        try:
            if adapts is None:
                classes, cls = fold_classes(self.param_groups, list(zip(gis, steps)))
            else:
                if any(ams):
                    raise ValueError("amsgrad is not supported together with trust_ratio (LAMB)")
                classes, cls, adapt_mask = fold_lamb_classes(self.param_groups, list(zip(gis, steps)), adapts)
            emas = ema.entries_of(plist) if ema is not None else None
            eng = self._bind(plist, states, ams, cls, emas)
            guard = self.skip_nonfinite
            if guard != getattr(eng, '_guard_on', False):       # the handle's switch: moved only when it has to
                _lib.check(eng.h, eng.lib.mc_optim_set_guard(eng.h, int(guard)), "mc_optim_set_guard")
                eng._guard_on = guard
        except Exception:
            self._step_cache = None             # nothing was stepped: the state's own counts are the truth again
            raise
        torch._foreach_add_([st['step'] for st in states], 1)   # in place: the tensors' identities (the cache key) survive
        if self.last_grad_norm is None:
            self.last_grad_norm = torch.zeros(1, dtype=torch.float32, device=plist[0].device)
        table = (_lib.OptimClass * len(classes))(*classes)
        max_norm = float(self.max_grad_norm) if self.max_grad_norm else 0.0
        norm_out = C.c_void_p(self.last_grad_norm.data_ptr())
        with torch.cuda.device(plist[0].device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)     # (the parameters' device's current stream)
            w = ema.weight() if ema is not None else 0.0
            if adapts is not None:
                who = "mc_clip_lamb_step_classes"
                rc = eng.lib.mc_clip_lamb_step_classes(eng.h, table, len(classes), adapt_mask, self.trust_clip, max_norm,
                                                       self.norm_type, w, norm_out, stream)
            elif ema is None:
                who = "mc_clip_adamw_step_classes"
                rc = eng.lib.mc_clip_adamw_step_classes(eng.h, table, len(classes), max_norm, self.norm_type, norm_out, stream)
            else:
                who = "mc_clip_adamw_ema_step_classes"
                rc = eng.lib.mc_clip_adamw_ema_step_classes(eng.h, table, len(classes), max_norm, self.norm_type, w, norm_out,
                                                            stream)
            _lib.check(eng.h, rc, who)
            if adapts is not None:
                self._ratio_params = plist      # the table mc_lamb_ratios reads
            if guard:                          # the device's verdict on this step, read whenever the caller gets to it
                self._step_calls += 1
                self._guard_reports.push(eng.lib, eng.h, stream, self._step_calls, plist)
        # the kernels updated the parameters behind torch's back: advance their version counters
        # (host-only bookkeeping) so autograd and the engine's packed-weight cache see the change
        torch.autograd.graph.increment_version(plist)
        if ema is not None:
            done = [e for e in emas if e is not None]
            if done:
                torch.autograd.graph.increment_version(done)
            # everything the pass above did not step: buffers, parameters without a gradient; counts the update
            # (guarded: a no-op on the device after a skipped step, so that the whole average stays where it was)
            ema.update_rest(ema.model, w, skip=frozenset(map(id, done)), engine=eng, guarded=guard)
        return loss


_CLIP_ENGINES = {}


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, engine=None, error_if_nonfinite=False):
    """``torch.nn.utils.clip_grad_norm_`` for contiguous float32 HIP gradients, as two multi-tensor launches and the
    one-wave final kernel: the total ``norm_type``-norm of all gradients (returned as a device scalar), every gradient
    scaled in place by ``min(1, max_norm / (norm + 1e-6))``.  The gradient table is bound to the engine's handle once
    and re-bound only when a gradient moved.  ``error_if_nonfinite=True`` is torch's argument: the norm is computed on its
    own first and read back (a synchronisation, as torch's), and a NaN or infinite one raises torch's ``RuntimeError``
    before any gradient is scaled."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None and p.grad.numel() > 0]
    p_norm = check_norm_type(norm_type)
    if not grads:
        return torch.tensor(0.0)
    dev = grads[0].device
    for g in grads:
        if g.dtype != torch.float32 or not g.is_cuda or g.device != dev or not g.is_contiguous():
            raise _lib.MonoconHipError("clip_grad_norm_ needs contiguous float32 HIP gradients on one device")
    eng = engine
    if eng is None:
        eng = _CLIP_ENGINES.get(dev.index)
        if eng is None:
            from hipmonocon.engine import Engine
            eng = _CLIP_ENGINES[dev.index] = Engine(dev.index)
    sig = tuple([(g.data_ptr(), g.numel()) for g in grads])
    if getattr(eng, '_clip_sig', None) != sig:
        n = len(grads)
        G, N = (C.c_void_p * n)(), (C.c_int64 * n)()
        for i, (ptr, numel) in enumerate(sig):
            G[i], N[i] = ptr, numel
        _lib.check(eng.h, eng.lib.mc_clip_bind(eng.h, n, G, N), "mc_clip_bind")
        eng._clip_sig = sig
    total = torch.zeros((), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if error_if_nonfinite:
            # max_norm 0: the norm passes alone, no gradient is touched
            rc = eng.lib.mc_clip_grad_norm(eng.h, 0.0, p_norm, C.c_void_p(total.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
            _lib.check(eng.h, rc, "mc_clip_grad_norm")
            if not bool(torch.isfinite(total)):
                raise RuntimeError(
                    "The total norm of order %s for gradients from `parameters` is non-finite, so it cannot be clipped. To "
                    "disable this error and scale the gradients by the non-finite norm anyway, set "
                    "`error_if_nonfinite=False`" % (norm_type,))
        rc = eng.lib.mc_clip_grad_norm(eng.h, float(max_norm), p_norm, C.c_void_p(total.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(eng.h, rc, "mc_clip_grad_norm")
    torch.autograd.graph.increment_version(grads)
    return total
