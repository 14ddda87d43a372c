"""Exponential moving average of a model's weights on MI355X (timm's ``ModelEmaV2``, mmdet's EMA hook, YOLO's ``ModelEMA``):
``e += (1 - decay_t) * (x - e)`` after every optimizer step, for evaluation and for the checkpoints.  The reference's train
loop has none; ``SOLVER.EMA.ENABLE`` turns it on (engine/monocon_engine.py).

One tensor per ``state_dict()`` entry of the model: floating-point entries (parameters and BatchNorm running statistics) are
averaged, integer entries (``num_batches_tracked``) are copied.  The average is formed by libmonocon_hip only, and in one
place (``ema_one``, csrc/kernels_optim.hip): by ``mc_ema_update`` -- one multi-tensor launch over a table of
(average, source) pairs -- or, for the parameters the fused AdamW steps, inside that step's own pass while the new value is
still in registers (``AdamW.set_ema``, solver/fused_adamw.py).  There is no torch fall-back: ``update()`` on CPU tensors
raises.
"""
import ctypes as C
import contextlib
from collections import OrderedDict

import torch

from hipmonocon import lib as _lib

WARMUP_NUM, WARMUP_DEN = 1.0, 10.0


class ModelEMA:
    """``ModelEMA(model, decay=0.9998, warmup=True, engine=None)``: the average starts as a copy of ``model``'s state.

    Stand-alone use: ``ema.update(model)`` after every ``optimizer.step()``.  Attached to the fused optimizer
    (``optimizer.set_ema(ema)``) the optimizer's ``step()`` does the whole update itself -- the stepped parameters inside the
    AdamW pass, everything else with one ``mc_ema_update`` -- and the caller does NOT call ``update``: it would average twice.
    """

    def __init__(self, model, decay=0.9998, warmup=True, engine=None):
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError("ModelEMA: decay must lie in [0, 1], got %r" % (decay,))
        self.decay, self.warmup, self.updates = float(decay), bool(warmup), 0
        self.model = model
        with torch.no_grad():
            self.tensors = OrderedDict((k, v.detach().clone()) for k, v in model.state_dict().items())
        self._engine = engine
        self._bound_sig = None
        self._entries = None            # entries_of's last answer

    # ------------------------------------------------------------------ schedule
    def decay_at(self, t):
        """decay of the update after ``t`` earlier ones: ``min(decay, (1 + t) / (10 + t))`` with warm-up (the early average
        follows the weights instead of their random start), else ``decay``"""
        if not self.warmup:
            return self.decay
        return min(self.decay, (WARMUP_NUM + t) / (WARMUP_DEN + t))

    def weight(self):
        """``w = 1 - decay_at(updates)`` of the next update, formed in double"""
        return 1.0 - self.decay_at(self.updates)

    # ------------------------------------------------------------------ update
    def set_engine(self, engine):
        self._engine = engine
        self._bound_sig = None

    def _live(self, model):
        live = model.state_dict()
        if live.keys() != self.tensors.keys():
            diff = sorted(set(live.keys()) ^ set(self.tensors.keys()))
            raise _lib.MonoconHipError("ModelEMA: the model's state_dict has other entries than the average (%s%s)"
                                       % (", ".join(diff[:4]), ", ..." if len(diff) > 4 else ""))
        return live

    def average(self, pairs, w, engine=None, guarded=False):
        """``e += w * (src - e)`` for every (e, src) of ``pairs`` in one ``mc_ema_update``; the table is re-bound only when a
        pointer moved.  ``guarded`` (the fused AdamW with ``skip_nonfinite``): ``mc_ema_update_guarded``, which does nothing
        on the device when the handle's last guarded step was skipped"""
        if not pairs:
            return
        dev = pairs[0][0].device
        for e, s in pairs:
            for t in (e, s):
                if t.dtype != torch.float32 or not t.is_cuda or t.device != dev or not t.is_contiguous():
                    raise _lib.MonoconHipError("ModelEMA needs contiguous float32 HIP tensors on one device (averages and "
                                               "model alike); libmonocon_hip has no CPU path")
            if e.numel() != s.numel():
                raise _lib.MonoconHipError("ModelEMA: an average and its source differ in size")
        eng = engine or self._engine
        if eng is None:
            from hipmonocon.engine import Engine
            eng = self._engine = Engine(dev.index)
        sig = tuple([(e.data_ptr(), s.data_ptr(), e.numel()) for e, s in pairs if e.numel() > 0])
        if not sig:
            return
        if sig != self._bound_sig or getattr(eng, '_ema_sig', None) is not self._bound_sig:
            n = len(sig)
            E, S, N = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int64 * n)()
            for i, (ep, sp, numel) in enumerate(sig):
                E[i], S[i], N[i] = ep, sp, numel
            _lib.check(eng.h, eng.lib.mc_ema_bind(eng.h, n, E, S, N), "mc_ema_bind")
            self._bound_sig = eng._ema_sig = sig
        with torch.cuda.device(dev):
            update = eng.lib.mc_ema_update_guarded if guarded else eng.lib.mc_ema_update
            rc = update(eng.h, float(w), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(eng.h, rc, "mc_ema_update_guarded" if guarded else "mc_ema_update")
        torch.autograd.graph.increment_version([e for e, _ in pairs])

    @torch.no_grad()
    def update_rest(self, model, w, skip=(), engine=None, guarded=False):
        """average every floating-point entry whose average is not in ``skip`` (ids of tensors of ``self.tensors`` that the
        fused optimizer has just averaged), copy the integer ones, count the update.  ``guarded``: after a skipped step the
        floating-point averages keep every bit; the update is counted and the integer entries (counters themselves) are
        copied all the same -- the host does not wait to learn the outcome"""
        live = self._live(model)
        pairs, copies = [], []
        for k, e in self.tensors.items():
            if id(e) in skip:
                continue
            (pairs if e.is_floating_point() else copies).append((e, live[k]))
        self.average(pairs, w, engine, guarded)     # (raises before anything is written)
        for e, s in copies:
            e.copy_(s)
        self.updates += 1

    def update(self, model=None):
        """one update of the whole average from ``model`` (default: the model given at construction).  Not to be called by a
        loop whose fused AdamW has this average attached: its ``step()`` has already done it."""
        self.update_rest(self.model if model is None else model, self.weight())

    def entries_of(self, params):
        """the average of each tensor of ``params`` (None where the model's state has no such floating-point entry), found
        by the identity of the model's own parameters"""
        key = tuple(map(id, params))
        if self._entries is not None and self._entries[0] == key and self._entries[1] is self.tensors:
            return self._entries[2]             # the same Parameter objects as last step: the same averages
        named = self.model.state_dict(keep_vars=True)
        by_id = {id(v): k for k, v in named.items()}
        out = []
        for p in params:
            k = by_id.get(id(p))
            e = self.tensors.get(k) if k is not None else None
            out.append(e if e is not None and e.is_floating_point() else None)
        self._entries = (key, self.tensors, out)
        return out

    # ------------------------------------------------------------------ state
    def state_dict(self):
        return {'tensors': OrderedDict(self.tensors), 'updates': self.updates, 'decay': self.decay, 'warmup': self.warmup}

    @torch.no_grad()
    def load_state_dict(self, state):
        src = state['tensors']
        if src.keys() != self.tensors.keys():
            diff = sorted(set(src.keys()) ^ set(self.tensors.keys()))
            raise KeyError("ModelEMA.load_state_dict: entries differ (%s%s)" % (", ".join(diff[:4]), ", ..." if len(diff) > 4 else ""))
        for k, e in self.tensors.items():
            e.copy_(src[k])                     # in place: the bound table keeps its pointers, the device stays
        self.updates, self.decay, self.warmup = int(state['updates']), float(state['decay']), bool(state['warmup'])

    @torch.no_grad()
    def reset_from(self, model):
        """start over from ``model``'s state (a checkpoint without an average)"""
        live = self._live(model)
        for k, e in self.tensors.items():
            e.copy_(live[k])
        self.updates = 0

    def to(self, device):
        self.tensors = OrderedDict((k, v.to(device)) for k, v in self.tensors.items())
        self._bound_sig = None
        return self

    # ------------------------------------------------------------------ use
    @torch.no_grad()
    def copy_to(self, model):
        """the averaged weights into ``model`` (torch copies: they advance the tensors' versions, so the engine's
        packed-weight cache refreshes on the next forward)"""
        live = self._live(model)
        for k, e in self.tensors.items():
            live[k].copy_(e)

    @contextlib.contextmanager
    def applied(self, model):
        """``with ema.applied(model): ...`` runs the body with the averaged weights in ``model`` and puts the live ones back,
        bit for bit, on the way out -- also when the body raises.  Torch copies on both sides (not the hot path): every
        tensor's version advances twice, so the packed-weight cache refreshes on the way in and on the way out."""
        with torch.no_grad():
            live = self._live(model)
            saved = OrderedDict((k, v.clone()) for k, v in live.items())
            self.copy_to(model)
        try:
            yield model
        finally:
            with torch.no_grad():
                for k, v in self._live(model).items():
                    v.copy_(saved[k])
