"""Autograd bridge of the HIP train step.

``forward_train(detector, data_dict)`` runs ``mc_forward_train`` (train-mode forward, target
generation, the ten losses) and returns ``(pred_dict, loss_dict)`` exactly like the reference's
``MonoConDetector.forward`` in train mode (model/detector/monocon_detector.py:53-61): the loss
values are 0-dim tensors connected to the model's parameters through one
``torch.autograd.Function`` whose ``backward`` calls ``mc_backward``, so the reference's train
loop (``sum(loss_dict.values()).backward()``, ``clip_grad_norm_``, ``optimizer.step()``,
engine/monocon_engine.py:84-102) runs unchanged on top of it.  The ten prediction maps are
differentiable outputs of the same Function: an objective that reaches them (an extra term on
``pred_dict``, ``head._get_losses`` against other targets) back-propagates through
``mc_backward_pred_grads``, which adds their gradients to the loss gradients in one pass.  The image
is a differentiable input too: when it requires a gradient the backward goes through
``mc_backward_image_grad`` and autograd receives d objective / d img (``img.grad`` of a leaf).
"""
import ctypes as C

import weakref

import torch

from . import dist as _dist
from . import lib as _lib
from . import netspec

PRED_KEYS = tuple(k for k, _ in netspec.PRED_KEYS)
PRED_CH = tuple(c for _, c in netspec.PRED_KEYS)
LABEL_FIELDS = ("gt_bboxes", "gt_labels", "gt_bboxes_3d", "depths", "gt_kpts_2d", "gt_kpts_valid_mask", "mask")
DEAD = frozenset(netspec.DEAD_PARAMS)


class _TrainBinding:
    """Per-detector bookkeeping: gradient buffers bound as '<key>#grad', BN buffer list."""

    def __init__(self, detector):
        self.named = [(n, p) for n, p in detector.named_parameters()]
        self.live = [(n, p) for n, p in self.named if n not in DEAD]
        # all live gradients in one contiguous buffer: the kernels write into its views, the data-
        # parallel all-reduce runs once over the whole buffer (hipmonocon/dist.py)
        self.flat = _dist.FlatGrads(self.live, self.named[0][1].device)
        self.grads = self.flat.views
        self.buffers = [b for _, b in detector.named_buffers()]
        self.sig = tuple(p.data_ptr() for _, p in self.named)

    def state(self, detector):
        st = dict(detector.state_dict(keep_vars=True))
        for n, g in self.grads.items():
            st[n + "#grad"] = g
        return st


def _binding(detector):
    tb = getattr(detector, "_train_binding", None)
    sig = tuple(p.data_ptr() for _, p in detector.named_parameters())
    if tb is None or tb.sig != sig:
        tb = _TrainBinding(detector)
        object.__setattr__(detector, "_train_binding", tb)
    return tb


def _loss_grad_vector(grads, like):
    """(10,) device vector of the upstream gradients of the ten losses (None: that loss does not reach the objective)"""
    first = grads[0]
    if first is not None and all(g is first for g in grads):        # sum(loss_dict.values()).backward(): one shared scalar
        return first.detach().reshape(1).expand(10).contiguous().float()
    zero = torch.zeros((), dtype=torch.float32, device=like.device)
    return torch.stack([zero if g is None else g.detach().reshape(()).float() for g in grads])


def _pred_grads(grads):
    """the upstream gradients of the ten prediction maps as fp32 contiguous tensors (None: that map does not reach the
    objective), or None when none does.  A gradient of pred.sum() arrives expanded (stride 0): contiguous() forms it."""
    if all(g is None for g in grads):
        return None
    return [None if g is None else g.detach().float().contiguous() for g in grads]


def _ptr_array(tensors):
    return (C.c_void_p * _lib.NUM_PREDS)(*[None if t is None else t.data_ptr() for t in tensors])


def _own_scalars(vec):
    """the entries of a device vector as 0-dim tensors with storage of their own (one multi-tensor copy)"""
    out = [torch.empty((), dtype=vec.dtype, device=vec.device) for _ in range(vec.numel())]
    torch._foreach_copy_(out, list(vec.unbind(0)))
    return out


class _HipTrainStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, detector, tb, eng, img, label, max_objs, *params):
        # a prediction map the objective does not use gets no gradient: left to its default, autograd hands backward() a
        # zero-filled tensor for each of them (255 MB of fills per step at B = 32, found in the kernel trace)
        ctx.set_materialize_grads(False)
        B, _, H, W = img.shape
        fh, fw = H // 4, W // 4
        preds = [torch.empty((B, c, fh, fw), dtype=torch.float32, device=img.device) for c in PRED_CH]
        losses = torch.zeros(10, dtype=torch.float32, device=img.device)
        lab = _lib.Labels()
        keep = []
        for f in LABEL_FIELDS:
            t = label[f]
            if not (t.is_cuda and t.dtype == torch.float32):
                raise _lib.MonoconHipError("label.%s must be a float32 HIP tensor (collate_fn contract)" % f)
            t = t.contiguous()
            keep.append(t)
            setattr(lab, f, t.data_ptr())
        arr = (C.c_void_p * _lib.NUM_PREDS)(*[p.data_ptr() for p in preds])
        with torch.cuda.device(img.device):
            rc = eng.lib.mc_forward_train(eng.h, C.c_void_p(img.data_ptr()), C.byref(lab), B, H, W, int(max_objs), arr,
                                          C.c_void_p(losses.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(eng.h, rc, "mc_forward_train")
        gen = C.c_ulonglong(0)
        _lib.check(eng.h, eng.lib.mc_train_generation(eng.h, C.byref(gen)), "mc_train_generation")
        ctx.generation = gen.value
        torch.autograd.graph.increment_version(tb.buffers)        # running statistics were updated in place
        ctx.eng, ctx.tb, ctx.keep, ctx.detector = eng, tb, (img, keep, losses), detector
        # the maps are differentiable outputs, and the backward reads them (loss gradients, activation derivatives):
        # saved as such, an in-place edit of one before backward() raises autograd's version error
        ctx.save_for_backward(*preds)
        # ten separate 0-dim outputs: the backward then receives the ten upstream gradients directly, instead of ten
        # select-backward nodes each filling a zero vector and adding it.  They own their storage (one multi-tensor copy
        # out of the device vector the kernel wrote): as outputs that are views of one buffer, an in-place loss weighting
        # (loss_dict[k] *= w) would trip autograd's "output of a function that returns multiple views" check
        return (*_own_scalars(losses), *preds)

    @staticmethod
    def backward(ctx, *grads):
        eng, tb = ctx.eng, ctx.tb
        ctx.saved_tensors                    # (unpacking checks that no map was modified in place since the forward)
        grad_losses = _loss_grad_vector(grads[:10], ctx.keep[2])
        gen = C.c_ulonglong(0)
        _lib.check(eng.h, eng.lib.mc_train_generation(eng.h, C.byref(gen)), "mc_train_generation")
        if gen.value != ctx.generation:
            raise _lib.MonoconHipError(
                "backward of train forward #%d, but the handle's saved activations belong to forward #%d: the HIP train "
                "plan keeps one set of activations, so call backward() before the next forward (for gradient "
                "accumulation run forward+backward per micro-batch)" % (ctx.generation, gen.value))
        g = grad_losses.contiguous().float()
        gp = _pred_grads(grads[10:])
        # the image asks for its gradient (a leaf with requires_grad_(), or the output of something that does): the stem's
        # data gradient runs as one more step of the backward and writes it here; otherwise the calls are the usual ones
        gimg = torch.empty_like(ctx.keep[0]) if ctx.needs_input_grad[3] else None
        with torch.cuda.device(g.device):
            if gimg is not None:
                what = "mc_backward_image_grad"
                rc = eng.lib.mc_backward_image_grad(eng.h, C.c_void_p(g.data_ptr()), None if gp is None else _ptr_array(gp),
                                                    C.c_void_p(gimg.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            elif gp is None:
                what = "mc_backward"
                rc = eng.lib.mc_backward(eng.h, C.c_void_p(g.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            else:
                what = "mc_backward_pred_grads"
                rc = eng.lib.mc_backward_pred_grads(eng.h, C.c_void_p(g.data_ptr()), _ptr_array(gp),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(eng.h, rc, what)
        # data parallel: with a communicator owned by the handle mc_backward already exchanged the gradients bucket by
        # bucket, overlapped with the backbone's backward (csrc/mc_comm.hip); otherwise one all-reduce of the flat buffer
        # (defer_grad_exchange: none of it -- the caller accumulates a window and calls exchange_grads_now once)
        if getattr(ctx.detector, "_defer_grad_exchange", False):
            pass
        elif eng.comm_world:
            if not eng.comm_info()["overlap"]:
                eng.allreduce_grads()
        else:
            tb.flat.allreduce_mean()
        out = []
        for n, p in tb.named:
            gb = tb.grads.get(n)
            if gb is None:
                out.append(None)
            elif p.grad is None:
                # a fresh alias (use_count 1): AccumulateGrad adopts it as p.grad -- a view of the flat
                # buffer, no copy; returning the stored view object itself would make torch clone it
                out.append(gb.detach())
            else:
                out.append(gb.clone())    # caller is accumulating across backward passes: torch adds a copy
        return (None, None, None, gimg, None, None, *out)


def _require_objects(detector, label, pad_hw, num_classes=3):
    """The reference asserts on empty targets (losses/l1_loss.py:15, README.MD:208-210) and fails with an index
    error for an object whose centre falls outside the feature map or whose class id is out of range
    (utils/target_generator.py:70-75: the heat-map / gather index is out of bounds); so does this path, before
    anything is launched.  One deliberate divergence: a NEGATIVE class id raises here, while the reference's Python
    indexing wraps it silently (class -1 would splat into the last heat-map channel) -- a label error either way.  Reading the verdict back is a host sync, so a label set that was already validated
    (the SAME mask tensor object, unmodified: a resident batch stepped repeatedly) is not read back again."""
    mask = label["mask"]
    seen = getattr(detector, "_mask_validated", None)
    cached = seen is not None and seen[0]() is mask and seen[1] == mask._version
    # Data parallel: whether the verdict has to be read back is a per-rank fact (one rank re-uses its label tensors, another
    # feeds fresh ones: an uneven tail, a retry), but the collective that lets all ranks raise together must be entered by
    # ALL of them or none (a rank that skipped it left the others waiting).  So every step votes first on "is
    # everybody's mask already validated" -- over the host-side group (gloo between the hosts, ~0.1 ms, no device work and
    # no stream sync: the host keeps running ahead of the GPU; ADVICE r3 was about a vote that synchronised the stream) --
    # and only when somebody's is not do all ranks enter the verdict's collective, the validated ones with (True, True).
    dp = _dist.is_distributed()
    if dp and _dist.host_votes_are_cheap():
        all_cached, = _dist.all_ranks_ok_many((cached,), mask.device, host=True)
        if all_cached:
            return
    elif cached:
        # single process -- or data parallel WITHOUT a host-side group (gloo unavailable beside nccl): a vote on
        # device tensors would synchronise the stream in front of the overlapped gradient exchange on every step, so the
        # round-3 contract applies instead: a label set validated on this rank is not voted on again (warned once)
        return
    H, W = pad_hw
    fh, fw = H // 4, W // 4
    n_valid, n_bad = 1, 0
    if not cached:      # (a rank whose labels are validated joins the others' collective with a clean verdict)
        bb, cls = label["gt_bboxes"], label["gt_labels"]
        # same fp32 arithmetic as make_targets_kernel: centre = (x1 + x2) * (fw / W) / 2, truncated toward zero
        wr = torch.tensor(fw / W, dtype=torch.float32, device=bb.device)
        hr = torch.tensor(fh / H, dtype=torch.float32, device=bb.device)
        xi = ((bb[..., 0] + bb[..., 2]) * wr / 2.0).trunc()
        yi = ((bb[..., 1] + bb[..., 3]) * hr / 2.0).trunc()
        bad = ((xi < 0) | (xi >= fw) | (yi < 0) | (yi >= fh) | (cls < 0) | (cls >= num_classes)) & (mask != 0)
        n_valid, n_bad = torch.stack([mask.sum(), bad.sum().to(mask.dtype)]).tolist()
    # data parallel: every rank raises together (a lone raise would leave the others in the all-reduce); both verdicts
    # travel in ONE two-element MIN all-reduce
    ok_valid, ok_inside = _dist.all_ranks_ok_many((n_valid != 0, n_bad == 0), mask.device, host=True)
    if not ok_valid:
        raise AssertionError("no valid objects in the batch: l1_loss requires target.numel() > 0")
    if not ok_inside:
        raise IndexError("%s with a box centre outside the %dx%d feature map or a class id outside "
                         "[0, %d): the reference's target generator indexes out of bounds for such labels"
                         % (("%d labelled object(s)" % int(n_bad)) if n_bad else "labelled object(s) on another rank", fh, fw, num_classes))
    object.__setattr__(detector, "_mask_validated", (weakref.ref(mask), mask._version))


def labels_ok_on_host(label, pad_hw, num_classes=3):
    """_require_objects' test on label tensors that are still in HOST memory (a DataLoader batch before its upload): the same
    fp32 arithmetic, no device work and no read-back.  True only for a batch the device-side test would pass; for anything
    else (labels already on a device, no valid object, an object outside the map or the classes) False -- the caller then
    leaves the batch to _require_objects, which raises as the reference does, on every rank together."""
    mask = label["mask"]
    if mask.is_cuda or label["gt_bboxes"].is_cuda or label["gt_labels"].is_cuda:
        return False
    H, W = pad_hw
    fh, fw = H // 4, W // 4
    bb, cls = label["gt_bboxes"].float(), label["gt_labels"]
    wr, hr = torch.tensor(fw / W, dtype=torch.float32), torch.tensor(fh / H, dtype=torch.float32)
    xi = ((bb[..., 0] + bb[..., 2]) * wr / 2.0).trunc()
    yi = ((bb[..., 1] + bb[..., 3]) * hr / 2.0).trunc()
    bad = ((xi < 0) | (xi >= fw) | (yi < 0) | (yi >= fh) | (cls < 0) | (cls >= num_classes)) & (mask != 0)
    return bool(mask.sum() != 0) and not bool(bad.any())


def note_labels_validated(detector, label):
    """the device copy ``label`` of a batch that labels_ok_on_host passed: _require_objects will not read a verdict back for
    it (under data parallelism the ranks still vote, over the host-side group, on whether all of them are in that state)"""
    mask = label["mask"]
    object.__setattr__(detector, "_mask_validated", (weakref.ref(mask), mask._version))


def _hold_overlap(detector, eng):
    """deferral is on: switch the handle's in-backward exchange off, once, remembering what it was"""
    if eng is None or not eng.comm_world or getattr(detector, "_deferred_overlap", None) is not None:
        return
    was = eng.comm_info()["overlap"]
    eng.comm_set_overlap(False)
    object.__setattr__(detector, "_deferred_overlap", (eng, was))


def defer_grad_exchange(detector, on):
    """What DDP's ``no_sync`` does, for a loop that accumulates gradients over a window of micro-batches
    (``solver.GradAccumulator``): while on, the backward of ``detector`` exchanges nothing -- neither ``mc_allreduce_grads``
    nor the flat buffer's all-reduce -- and the handle's exchange overlapped with the backward is switched off
    (``mc_comm_set_overlap(h, 0)``).  Turning it off restores the overlap setting that was found.  The mean over ranks
    commutes with the sum over micro-batches, so ONE ``exchange_grads_now`` on the window's mean replaces one exchange per
    micro-batch; it is not overlapped with any backward."""
    on = bool(on)
    object.__setattr__(detector, "_defer_grad_exchange", on)
    if on:
        _hold_overlap(detector, detector._rt.engine)
        return
    held = getattr(detector, "_deferred_overlap", None)
    if held is not None:
        object.__setattr__(detector, "_deferred_overlap", None)
        eng, was = held
        if eng.comm_world:                  # (the communicator may have been destroyed meanwhile)
            eng.comm_set_overlap(was)


def exchange_grads_now(detector):
    """the one gradient exchange a backward without overlap performs, on what the gradient buffer holds now:
    ``mc_allreduce_grads`` when the handle owns a communicator, else the all-reduce of the flat buffer through
    torch.distributed -- which is nothing outside a distributed run.  For a window accumulated under ``defer_grad_exchange``."""
    tb = getattr(detector, "_train_binding", None)
    eng = detector._rt.engine
    if tb is None or eng is None:
        raise _lib.MonoconHipError("exchange_grads_now: the detector has not run a train step yet (no gradient buffer is bound)")
    if eng.comm_world:
        eng.allreduce_grads()
    else:
        tb.flat.allreduce_mean()


def forward_train(detector, data_dict):
    img = data_dict["img"]
    if not img.is_cuda:
        raise _lib.MonoconHipError("img must live on a HIP device; libmonocon_hip has no CPU path")
    label = data_dict["label"]
    _require_objects(detector, label, img.shape[-2:])
    tb = _binding(detector)
    for n, p in tb.live:
        # a .grad that still aliases the flat buffer (zero_grad(set_to_none=False)) would be overwritten
        # by the kernels before torch can accumulate into it: give torch its own copy in that case
        if p.grad is not None and p.grad.data_ptr() == tb.grads[n].data_ptr():
            p.grad = p.grad.clone()
    eng = detector._rt.get(tb.state(detector))
    if _dist.is_distributed():
        _dist.setup_engine_dp(eng, img.shape[0], img.shape[2], img.shape[3])      # collective, once per engine (its first step)
    if getattr(detector, "_defer_grad_exchange", False):
        _hold_overlap(detector, eng)       # (a communicator that was built just now starts with its overlap on)
    params = [p for _, p in tb.named]
    out = _HipTrainStep.apply(detector, tb, eng, img.contiguous(), label, detector.head.max_objs, *params)
    losses, preds = out[:10], out[10:]
    pred_dict = dict(zip(PRED_KEYS, preds))
    loss_dict = {k: losses[i] for i, k in enumerate(netspec.LOSS_KEYS)}
    return pred_dict, loss_dict


# ----------------------------------------------------------------------------- heads on their own
class _HeadBinding:
    """gradient buffers of a stand-alone MonoConDenseHeads, bound as 'head.<key>#grad'"""

    def __init__(self, heads):
        self.named = [("head." + n, p) for n, p in heads.named_parameters()]
        self.flat = _dist.FlatGrads(self.named, self.named[0][1].device)
        self.grads = self.flat.views
        self.buffers = [b for _, b in heads.named_buffers()]
        self.sig = tuple(p.data_ptr() for _, p in self.named)

    def state(self, heads):
        st = {"head." + k: v for k, v in heads.state_dict(keep_vars=True).items()}
        for n, g in self.grads.items():
            st[n + "#grad"] = g
        return st


class _HipHeadTrainStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tb, eng, feat, label, pad_hw, max_objs, *params):
        ctx.set_materialize_grads(False)       # (see _HipTrainStep.forward)
        B, _, fh, fw = feat.shape
        preds = [torch.empty((B, c, fh, fw), dtype=torch.float32, device=feat.device) for c in PRED_CH]
        losses = torch.zeros(10, dtype=torch.float32, device=feat.device)
        lab = _lib.Labels()
        keep = []
        for f in LABEL_FIELDS:
            t = label[f]
            if not (t.is_cuda and t.dtype == torch.float32):
                raise _lib.MonoconHipError("label.%s must be a float32 HIP tensor (collate_fn contract)" % f)
            t = t.contiguous()
            keep.append(t)
            setattr(lab, f, t.data_ptr())
        arr = (C.c_void_p * _lib.NUM_PREDS)(*[p.data_ptr() for p in preds])
        with torch.cuda.device(feat.device):
            rc = eng.lib.mc_head_forward_train(eng.h, C.c_void_p(feat.data_ptr()), C.byref(lab), B, int(pad_hw[0]), int(pad_hw[1]),
                                               int(max_objs), arr, C.c_void_p(losses.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(eng.h, rc, "mc_head_forward_train")
        gen = C.c_ulonglong(0)
        _lib.check(eng.h, eng.lib.mc_train_generation(eng.h, C.byref(gen)), "mc_train_generation")
        ctx.generation = gen.value
        torch.autograd.graph.increment_version(tb.buffers)
        ctx.eng, ctx.tb, ctx.keep, ctx.feat_shape = eng, tb, (feat, keep, losses), feat.shape
        ctx.save_for_backward(*preds)          # (see _HipTrainStep.forward)
        return (*_own_scalars(losses), *preds)

    @staticmethod
    def backward(ctx, *grads):
        eng, tb = ctx.eng, ctx.tb
        ctx.saved_tensors
        grad_losses = _loss_grad_vector(grads[:10], ctx.keep[2])
        gen = C.c_ulonglong(0)
        _lib.check(eng.h, eng.lib.mc_train_generation(eng.h, C.byref(gen)), "mc_train_generation")
        if gen.value != ctx.generation:
            raise _lib.MonoconHipError("backward of head forward #%d, but the handle's saved activations belong to forward "
                                       "#%d: call backward() before the next forward_train" % (ctx.generation, gen.value))
        g = grad_losses.contiguous().float()
        gfeat = torch.empty(ctx.feat_shape, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[2] else None
        gp = _pred_grads(grads[10:])
        with torch.cuda.device(g.device):
            if gp is None:
                rc = eng.lib.mc_head_backward(eng.h, C.c_void_p(g.data_ptr()), C.c_void_p(gfeat.data_ptr() if gfeat is not None else None),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
            else:
                rc = eng.lib.mc_head_backward_pred_grads(eng.h, C.c_void_p(g.data_ptr()), _ptr_array(gp),
                                                         C.c_void_p(gfeat.data_ptr() if gfeat is not None else None),
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(eng.h, rc, "mc_head_backward" if gp is None else "mc_head_backward_pred_grads")
        out = []
        for n, p in tb.named:
            gb = tb.grads[n]
            out.append(gb.detach() if p.grad is None else gb.clone())
        return (None, None, gfeat, None, None, None, *out)


def head_forward_train(heads, feat, data_dict):
    """``MonoConDenseHeads.forward_train(feat, data_dict)`` of the reference (monocon_heads.py:150-157): targets,
    train-mode predictions and the ten losses from a neck output, autograd-connected to ``feat`` and to the head's
    parameters.  (Inside MonoConDetector the whole network runs as one plan; this is the stand-alone entry.)"""
    if not feat.is_cuda:
        raise _lib.MonoconHipError("feat must live on a HIP device; libmonocon_hip has no CPU path")
    label = data_dict["label"]
    pad_hw = data_dict["img_metas"]["pad_shape"][0]
    if tuple(feat.shape[1:]) != (64, int(pad_hw[0]) // 4, int(pad_hw[1]) // 4):
        raise _lib.MonoconHipError("feat %s does not match pad_shape %s (expected (B,64,H/4,W/4))" % (tuple(feat.shape), tuple(pad_hw)))
    _require_objects(heads, label, pad_hw)
    tb = getattr(heads, "_train_binding", None)
    sig = tuple(p.data_ptr() for _, p in heads.named_parameters())
    if tb is None or tb.sig != sig:
        tb = _HeadBinding(heads)
        object.__setattr__(heads, "_train_binding", tb)
    for n, p in tb.named:
        if p.grad is not None and p.grad.data_ptr() == tb.grads[n].data_ptr():
            p.grad = p.grad.clone()
    eng = heads._rt.get(tb.state(heads))
    params = [p for _, p in tb.named]
    out = _HipHeadTrainStep.apply(tb, eng, feat.contiguous().float(), label, pad_hw, heads.max_objs, *params)
    losses, preds = out[:10], out[10:]
    return dict(zip(PRED_KEYS, preds)), {k: losses[i] for i, k in enumerate(netspec.LOSS_KEYS)}
