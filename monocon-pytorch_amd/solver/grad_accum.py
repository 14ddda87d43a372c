"""Gradient accumulation over a window of micro-batches on MI355X: several ``backward()`` calls, one ``optimizer.step()``.

``mc_backward`` WRITES the gradient tensors (the ``.grad`` of every parameter aliases the engine's flat gradient buffer), so
a second ``backward()`` before a step would overwrite the first one's result; torch's own accumulation works only through a
clone of every gradient and one add per tensor (hipmonocon/train.py).  ``GradAccumulator`` keeps the running sum beside the
gradients instead, in one flat buffer of its own, and drives ``mc_grad_accumulate`` (csrc/kernels_optim.hip): ONE launch
after each micro-batch's backward, and after the window's last one the gradients themselves hold the window's MEAN -- the
clip, the fused AdamW, the non-finite guard, the weight average and the gradient exchange then run unchanged.

    acc = GradAccumulator(model.parameters(), steps=4)
    for i, batch in enumerate(loader):
        optimizer.zero_grad()                     # set_to_none: .grad stays the alias of the flat buffer, no copy anywhere
        _, loss_dict = model(batch)
        sum(loss_dict.values()).backward()        # the UNSCALED loss of the micro-batch
        if acc.accumulate(last=(i + 1 == len(loader))):
            optimizer.step()                      # p.grad is the mean over the window

Loss convention: the accumulator AVERAGES over the window, so every micro-batch back-propagates its loss as it is -- not
``loss / steps`` (that would divide twice).  A window of k micro-batches of b images is then the gradient of the mean loss over
k * b images, which is what data parallelism over k ranks computes (BatchNorm statistics per micro-batch, as per replica there).

The epoch's tail: a window never spans epochs.  The caller -- who knows ``len(loader)`` -- passes ``last=True`` with the true
last micro-batch, and the window closes there with its own count (``scale = 1 / pending``).  That is the one way to close a
shorter window: after ``accumulate()`` has returned False the last gradient is already part of the sum, and turning the sum
into the mean would take a further kernel mode; ``flush()`` therefore only answers False when nothing is pending and raises on
an open window, naming ``last=True``.

Launches of a window of k micro-batches: k = 1 none at all (``steps=1`` is the plain loop exactly), k = 2 BEGIN, FINISH(1/2),
k >= 3 BEGIN, ADD x (k - 2), FINISH(1/k).  There is no torch fall-back.
"""
import operator

import torch

from hipmonocon import lib as _lib


def window_modes(k):
    """the (mode, scale) launches of a window of ``k`` micro-batches, in order (scale None: the mode ignores it)"""
    if k < 2:
        return []
    return [(_lib.ACCUM_BEGIN, None)] + [(_lib.ACCUM_ADD, None)] * (k - 2) + [(_lib.ACCUM_FINISH, 1.0 / k)]


def optimizer_steps_per_epoch(num_batches, steps):
    """optimizer steps of an epoch of ``num_batches`` micro-batches: full windows of ``steps`` and one shorter tail window"""
    return -(-int(num_batches) // int(steps))


class GradAccumulator:
    """``GradAccumulator(params, steps=N, engine=None)``; see the module's text.  ``engine``: a ``hipmonocon.engine.Engine`` (or
    anything with its ``accum_bind(grads, accs)`` and ``grad_accumulate(mode, scale)``); None: one of its own, made at the first
    launch on the gradients' device."""

    def __init__(self, params, steps, engine=None):
        if isinstance(steps, bool):
            raise TypeError("GradAccumulator: steps must be an integer, got %r" % (steps,))
        try:
            steps = operator.index(steps)
        except TypeError:
            raise TypeError("GradAccumulator: steps must be an integer, got %r" % (steps,)) from None
        if steps < 1:
            raise ValueError("GradAccumulator: steps must be >= 1, got %d" % steps)
        self.steps = steps
        self.params = [params] if torch.is_tensor(params) else list(params)
        self._engine = engine
        self.pending = 0                # micro-batches in the open window
        self.flat = None                # the accumulators: one allocation, every slice at a multiple of 4 floats
        self.offsets, self.slices = [], []
        self._bound_sig = None

    def set_engine(self, engine):
        if self.pending:
            raise _lib.MonoconHipError("GradAccumulator: the engine cannot change inside an open window")
        self._engine = engine
        self._bound_sig = None

    # ------------------------------------------------------------------ table
    def _grads(self):
        return [p.grad for p in self.params if p.grad is not None]

    def _bind(self, grads, sig):
        """the table: the parameters with a gradient, in the order of ``params`` (the optimizer's)"""
        for g in grads:
            if g.dtype != torch.float32 or g.device != grads[0].device or not g.is_contiguous():
                raise _lib.MonoconHipError("GradAccumulator needs contiguous float32 gradients on one device")
        eng = self._engine
        if eng is None:
            from hipmonocon.engine import Engine
            eng = self._engine = Engine(grads[0].device.index)
        offsets, total = [], 0
        for g in grads:
            offsets.append(total)
            total += (g.numel() + 3) // 4 * 4
        if self.flat is None or self.flat.numel() != total or self.flat.device != grads[0].device:
            self.flat = torch.zeros(total, dtype=torch.float32, device=grads[0].device)
        self.offsets = offsets
        self.slices = [self.flat[o:o + g.numel()] for o, g in zip(offsets, grads)]
        eng.accum_bind(grads, self.slices)
        self._bound_sig = eng._accum_sig = sig
        return eng

    # ------------------------------------------------------------------ window
    @torch.no_grad()
    def accumulate(self, last=False):
        """after the ``backward()`` of a micro-batch.  True: the window is complete -- ``steps`` micro-batches, or fewer with
        ``last`` -- and every ``p.grad`` holds its mean: step now.  False: the gradients were added to the sum; run the next
        micro-batch (``zero_grad()`` first, so that ``.grad`` stays the alias mc_backward writes)."""
        i = self.pending + 1
        complete = i >= self.steps or bool(last)
        if i == 1 and complete:
            return True                 # a window of one: the gradient is its own mean, nothing is launched
        grads = self._grads()
        if not grads:
            raise _lib.MonoconHipError("GradAccumulator: no parameter has a gradient (accumulate() follows backward())")
        sig = tuple([(g.data_ptr(), g.numel()) for g in grads])
        eng = self._engine
        bound = sig == self._bound_sig and getattr(eng, '_accum_sig', None) is self._bound_sig
        if i == 1:
            if not bound:               # re-bound only when a gradient moved (or another accumulator used the handle)
                eng = self._bind(grads, sig)
            eng.grad_accumulate(_lib.ACCUM_BEGIN)
            self.pending = 1
            return False
        if not bound:
            # binding again would close the window on the handle, and a silent restart would drop what was accumulated
            raise _lib.MonoconHipError(
                "GradAccumulator: a gradient tensor moved (or the engine's table was re-bound) inside an open window of %d "
                "micro-batch(es); keep p.grad the alias the backward writes: zero_grad() (set to none) before every "
                "micro-batch, nothing that replaces p.grad in between" % self.pending)
        if not complete:
            eng.grad_accumulate(_lib.ACCUM_ADD)
            self.pending = i
            return False
        eng.grad_accumulate(_lib.ACCUM_FINISH, 1.0 / i)
        self.pending = 0
        # the kernel wrote the gradients behind torch's back (as clip_grad_norm_ does)
        torch.autograd.graph.increment_version(grads)
        return True

    def flush(self):
        """False when no window is open.  An open window cannot be closed from here (its last gradient is already part of the
        sum): pass ``last=True`` to ``accumulate()`` with the epoch's last micro-batch instead."""
        if not self.pending:
            return False
        raise _lib.MonoconHipError(
            "GradAccumulator.flush: %d micro-batch(es) are pending; a shorter window is closed by accumulate(last=True) on "
            "its last micro-batch (windows never span epochs), not afterwards" % self.pending)
