"""MonoconEngine: the reference's train / evaluate loop (engine/monocon_engine.py:23-194) on top of
the MI355X hot path.  ``train_one_epoch`` is the reference's step sequence -- zero_grad, H2D,
``self.model(data_dict)``, ``sum(losses).backward()``, clip, ``optimizer.step()``,
``scheduler.step()``, periodic logging -- with the clip folded into the fused HIP AdamW and, under
``torch.distributed.run``, a sharded sampler + the in-backward RCCL gradient all-reduce.

Data-parallel policy (N ranks): ``DATA.BATCH_SIZE`` is the PER-RANK batch (global batch = N x BATCH_SIZE),
the sampler shards the training set so an epoch has 1/N as many steps and the one-cycle schedule's
``total_steps`` shrinks with it; ``SOLVER.OPTIM.LR`` is used exactly as configured -- nothing is scaled
automatically, scale it in the config if the larger global batch calls for it.  All ranks start from rank 0's
weights (``hipmonocon.dist.sync_module_state``); rank 0 alone evaluates and writes checkpoints.
``SOLVER.NONFINITE_GUARD`` needs no collective: every rank steps on the same all-reduced gradients, computes the same norm
and takes the same decision to skip, so the replicas stay identical and every rank counts the same ``skipped_steps``.
``SOLVER.LAMB`` (off by default) makes the fused step LAMB: every tensor's update is rescaled by its trust ratio (solver/fused_adamw.py),
and the log line gains the min / median / max ratio of the step.  It adds no collective either -- the ranks form the same ratios from
the same parameters and gradients -- and it changes nothing about ``LR``: that is still used exactly as configured.

``SOLVER.ACCUM_STEPS`` N > 1 (default 1: the loop above, call for call): every optimizer step takes a window of N batches of
the loader -- micro-batches: zero_grad, forward, backward of the UNSCALED loss, one ``mc_grad_accumulate`` launch
(solver/grad_accum.py) -- and steps on the window's mean gradient; an epoch's last ``len(loader) % N`` batches form a shorter
window of their own, windows never span epochs.  Iterations, the log period, the schedule, the weight average and the guard's
reports count optimizer steps; the loss of a step is the mean of its micro-batches' losses.  Under data parallelism the
gradient exchange is deferred to the window's end: one exchange of the mean per step, not overlapped with a backward.
"""
import os
from typing import Dict, List

import torch
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from engine.base_engine import BaseEngine
from model import MonoConDetector
from solver import AdamW, CyclicScheduler, GradAccumulator, ModelEMA, build_param_groups
from solver.grad_accum import optimizer_steps_per_epoch
from utils.decorators import decorator_timer
from hipmonocon.feed import WORKER_CONTEXT, DeferredScalars, DevicePrefetcher, RingLoader, prepare_worker_context
from hipmonocon import train as hip_train
from utils.engine_utils import move_data_device, progress_to_string_bar, reduce_loss_dict, tprint


class _SeedWorker:
    """worker_init_fn (module level: the workers of a fork server get it pickled).  torch seeds numpy per WORKER from a base seed
    that is the same on every rank (replicas start from rank 0's seed): offset it per rank, or all ranks would draw the same
    augmentation decisions for their shards"""

    def __init__(self, rank):
        self.rank = rank

    def __call__(self, worker_id):
        import numpy as np
        np.random.seed((torch.initial_seed() + 1000003 * (self.rank + 1)) % (2 ** 32))


class MonoconEngine(BaseEngine):
    def __init__(self, cfg, **kwargs):
        super().__init__(cfg, **kwargs)

    def build_model(self):
        detector = MonoConDetector(num_dla_layers=self.cfg.MODEL.BACKBONE.NUM_LAYERS,
                                   pretrained_backbone=self.cfg.MODEL.BACKBONE.IMAGENET_PRETRAINED)
        return detector.to(self.current_device)

    def build_solver(self):
        assert self.model is not None and self.train_loader is not None
        clip, optim = self.cfg.SOLVER.CLIP_GRAD, self.cfg.SOLVER.OPTIM
        # group 0 is the base group (current_lr and the log line read it); BACKBONE_LR_MULT 1.0 and NO_DECAY_NORM_BIAS
        # False give the reference's single group.  BACKBONE_LR_MULT 0.0 freezes the backbone through the optimizer
        # only: its backward and its BatchNorm running statistics still run (solver/param_groups.py)
        groups = build_param_groups(self.model.named_parameters(), lr=optim.LR, weight_decay=optim.WEIGHT_DECAY,
                                    backbone_lr_mult=float(optim.get('BACKBONE_LR_MULT', 1.0)),
                                    no_decay_norm_bias=bool(optim.get('NO_DECAY_NORM_BIAS', False)))
        # SOLVER.NONFINITE_GUARD: the step skips itself on the device when the gradient norm is NaN or infinite
        # (solver/fused_adamw.py); train_one_epoch learns of it one step late, like the loss
        guard_cfg = self.cfg.SOLVER.get('NONFINITE_GUARD', None)
        # SOLVER.LAMB: the per-tensor trust ratio in the fused step (solver/fused_adamw.py); LR stays as configured
        lamb_cfg = self.cfg.SOLVER.get('LAMB', None)
        lamb = dict(trust_ratio=True, trust_clip=float(lamb_cfg.TRUST_CLIP), always_adapt=bool(lamb_cfg.ALWAYS_ADAPT)) \
            if lamb_cfg is not None and lamb_cfg.ENABLE else {}
        optimizer = AdamW(groups, lr=optim.LR, weight_decay=optim.WEIGHT_DECAY, betas=(0.95, 0.99),
                          max_grad_norm=float(clip.MAX_NORM) if clip.ENABLE else None,
                          norm_type=float(clip.NORM_TYPE) if clip.ENABLE else 2.0,
                          skip_nonfinite=bool(guard_cfg.ENABLE) if guard_cfg is not None else False, **lamb)
        # SOLVER.EMA: the optimizer's step keeps an average of the weights and BatchNorm statistics (solver/model_ema.py);
        # evaluate() runs on it and the checkpoints carry it.  Under data parallelism every rank keeps its own: the ranks
        # start from the same weights and apply the same all-reduced gradients, so the averages are identical and nothing
        # is exchanged; rank 0 saves.
        ema_cfg = self.cfg.SOLVER.get('EMA', None)
        if ema_cfg is not None and ema_cfg.ENABLE:
            self.ema = ModelEMA(self.model, decay=float(ema_cfg.DECAY), warmup=bool(ema_cfg.WARMUP))
            optimizer.set_ema(self.ema)
        # SOLVER.ACCUM_STEPS: N > 1 accumulates the gradients of N batches per optimizer step (solver/grad_accum.py); with 1
        # there is no accumulator and the loop is the reference's
        accum_steps = self.cfg.SOLVER.get('ACCUM_STEPS', 1)
        self.grad_accum = GradAccumulator(self.model.parameters(), steps=accum_steps) if accum_steps > 1 else None
        scheduler = None
        if self.cfg.SOLVER.SCHEDULER.ENABLE:
            # one schedule step per optimizer step: full windows and the epoch's shorter tail window
            total_steps = optimizer_steps_per_epoch(len(self.train_loader), accum_steps) * self.cfg.SOLVER.OPTIM.NUM_EPOCHS
            scheduler = CyclicScheduler(optimizer, total_steps=total_steps, target_lr_ratio=(10, 1E-04),
                                        target_momentum_ratio=(0.85 / 0.95, 1.0), period_up=0.4)
        return optimizer, scheduler

    def build_loader(self, is_train: bool = True):
        if str(self.cfg.DATA.ROOT).startswith('synthetic'):
            from dataset.synthetic_dataset import SyntheticMonoConDataset
            n = int(self.cfg.DATA.get('SYNTHETIC_LENGTH', 64))
            hw = self.cfg.DATA.get('SYNTHETIC_HW', (384, 1280))
            dataset = SyntheticMonoConDataset(length=n if is_train else max(n // 4, 1), height=int(hw[0]), width=int(hw[1]),
                                              max_objs=self.cfg.MODEL.HEAD.MAX_OBJS, seed=1 if is_train else 2)
        else:
            # the KITTI file dataset (dataset/monocon_dataset.py: PIL decode; the 'train' split runs the reference's random
            # augmentations, transforms/augmentations.py, every other split the deterministic list)
            from dataset.monocon_dataset import MonoConDataset
            # DATA.DEVICE_AUGMENT (default on beside a device): the samples carry the decoded uint8 frame + 24 parameters and the
            # detector forms the float32 frame on the device (mc_preprocess_augmented, bit-identical to the host transforms);
            # a worker then spends its time on the PNG and the labels, not on ~80 ms of float32 colour arithmetic per frame
            dataset = MonoConDataset(base_root=self.cfg.DATA.ROOT,
                                     split=self.cfg.DATA.TRAIN_SPLIT if is_train else self.cfg.DATA.TEST_SPLIT,
                                     max_objs=self.cfg.MODEL.HEAD.MAX_OBJS,
                                     filter_configs={k.lower(): v for k, v in dict(self.cfg.DATA.FILTER).items()},
                                     device_image=torch.cuda.is_available() and bool(self.cfg.DATA.get('DEVICE_AUGMENT', True)),
                                     resize_hw=list(self.cfg.DATA.get('RESIZE_HW', [])) or None)
        sampler = None
        if self.world > 1 and is_train:
            sampler = DistributedSampler(dataset, num_replicas=self.world, rank=self.rank, shuffle=True, drop_last=True)
        seed_worker = _SeedWorker(self.rank)
        if is_train and self.cfg.DATA.NUM_WORKERS == 0 and self.world > 1:
            seed_worker(0)
        shuffle, drop_last = (is_train and sampler is None), (self.world > 1 and is_train)
        init_fn = seed_worker if (is_train and self.cfg.DATA.NUM_WORKERS > 0) else None
        loader = None
        if self.cfg.DATA.NUM_WORKERS > 0 and torch.cuda.is_available() and bool(self.cfg.DATA.get('RING_LOADER', True)):
            # worker processes + a HIP device: the frames go through a shared, page-locked ring of batch slots instead of the
            # workers' queues (hipmonocon/feed.py: a DataLoader delivers a 32-frame float32 batch every 75-105 ms, the ring
            # every ~10).  Same batches in the same order; DATA.RING_LOADER: False is the reference's DataLoader.
            try:
                loader = RingLoader(dataset, self.cfg.DATA.BATCH_SIZE, self.cfg.DATA.NUM_WORKERS, shuffle=shuffle, sampler=sampler,
                                    drop_last=drop_last, collate_fn=dataset.collate_fn, worker_init_fn=init_fn)
            except (RuntimeError, OSError) as e:        # e.g. /dev/shm too small for the ring
                self._say("RingLoader unavailable (%s): using torch's DataLoader." % (e,))
        if loader is None:
            # pin_memory: a loader thread page-locks every batch, so that DevicePrefetcher's uploads are asynchronous -- and
            # beside page-locked memory the workers must not be forks of this process (hipmonocon/feed.py, RingLoader)
            beside_device = torch.cuda.is_available() and self.cfg.DATA.NUM_WORKERS > 0
            if beside_device:
                prepare_worker_context()
            loader = DataLoader(dataset, batch_size=self.cfg.DATA.BATCH_SIZE, num_workers=self.cfg.DATA.NUM_WORKERS,
                                shuffle=shuffle, sampler=sampler, collate_fn=dataset.collate_fn, drop_last=drop_last,
                                pin_memory=torch.cuda.is_available(), worker_init_fn=init_fn,
                                multiprocessing_context=WORKER_CONTEXT if beside_device else None,
                                persistent_workers=beside_device)
        return dataset, loader

    @decorator_timer
    def train_one_epoch(self) -> float:
        epoch_losses = []
        if hasattr(getattr(self.train_loader, 'sampler', None), 'set_epoch'):      # DistributedSampler (RingLoader shows it guarded)
            self.train_loader.sampler.set_epoch(self.epochs)
        # the batches arrive on the device one step ahead (copy stream, labels checked on the host) and the loss of a step is
        # read back while the NEXT one runs: nothing between two log lines drains the stream (hipmonocon/feed.py)
        losses = DeferredScalars()
        guarded = bool(getattr(self.optimizer, 'skip_nonfinite', False))
        lamb = bool(getattr(self.optimizer, 'trust_ratio', False))
        iters = []                  # global iteration numbers of the steps whose loss has not been read yet

        def collect(keep):
            got = losses.ready(keep)
            if guarded:
                # the guard's reports ride behind the losses, one per step: a skipped step is logged, its loss left out
                reports = self.optimizer.drain_guard_reports(keep)
                assert len(reports) == len(got), (len(reports), len(got))
                got = self.account_steps(iters[:len(got)], got, reports)
                del iters[:len(reports)]
            epoch_losses.extend(got)
            self.entire_losses.extend(got)

        # MONOCON_HIP_SYNC_LOOP=1: the reference's loop as written (upload on the compute stream, loss read inside the step)
        sync_loop = os.environ.get("MONOCON_HIP_SYNC_LOOP", "0") == "1"
        feed = self.train_loader if sync_loop else DevicePrefetcher(self.train_loader, self.current_device, self.model)
        # SOLVER.ACCUM_STEPS > 1: a window of micro-batches per optimizer step; everything below the `continue` runs once per
        # window.  The ranks' exchange waits for the window's mean (one exchange per step instead of one per micro-batch)
        accum = self.grad_accum
        deferred = accum is not None and self.world > 1
        if deferred:
            hip_train.defer_grad_exchange(self.model, True)
        n_batches = len(self.train_loader)
        window = []                 # the total losses of the open window's micro-batches (device scalars)
        try:
            for batch_idx, data_dict in enumerate(feed):
                self.optimizer.zero_grad()
                data_dict = move_data_device(data_dict, self.current_device)      # (a no-op for what the prefetcher uploaded)
                _, loss_dict = self.model(data_dict)
                total_loss = reduce_loss_dict(loss_dict)
                total_loss.backward()                       # HIP backward + (N > 1) gradient all-reduce
                if accum is not None:
                    window.append(total_loss.detach())
                    if not accum.accumulate(last=batch_idx + 1 == n_batches):
                        continue                            # the window is still open: the next micro-batch
                    if deferred:
                        hip_train.exchange_grads_now(self.model)
                    # the step's loss: the mean over its micro-batches, formed on the device (nothing is read back here)
                    total_loss = torch.stack(window).mean() if len(window) > 1 else window[0]
                    window = []
                losses.push(total_loss)
                if guarded:
                    iters.append(self.global_iters)
                self.optimizer.step()                       # fused clip (SOLVER.CLIP_GRAD) + AdamW
                if self.scheduler is not None:
                    self.scheduler.step()
                logging = self.global_iters % self.log_period == 0 and self.is_main
                collect(0 if (logging or sync_loop) else 1)
                if logging:
                    bar = progress_to_string_bar(batch_idx + 1, len(self.train_loader), bins=20)
                    last = self.entire_losses[-100:] or [float('nan')]      # (empty: every step so far was skipped)
                    recent = sum(last) / len(last)
                    print("| Progress %s | LR %.6f | Loss %8.4f (%8.4f) |" % (bar, self.current_lr, last[-1], recent))
                    if lamb:                                # SOLVER.LAMB: the adapting tensors' ratios of this step
                        r = sorted(self.optimizer.trust_ratios(adapting_only=True).values())
                        if r:
                            print("| Trust ratio | min %.4g | median %.4g | max %.4g |" % (r[0], r[len(r) // 2], r[-1]))
                    self._update_dict_to_writer(loss_dict, tag='loss')
                self._iter_update()
        finally:
            if deferred:
                hip_train.defer_grad_exchange(self.model, False)
        if accum is not None and accum.pending:
            raise RuntimeError("the train loader delivered fewer than its %d batches: a window of %d micro-batch(es) is still open "
                               "at the end of the epoch, and windows never span epochs" % (n_batches, accum.pending))
        collect(0)
        self._epoch_update()
        return sum(epoch_losses) / max(len(epoch_losses), 1)

    @torch.no_grad()
    def evaluate(self) -> Dict[str, float]:
        if self.ema is None:
            return self._evaluate_model()
        # SOLVER.EMA: on the averaged weights; the live ones are back, bit for bit, when this returns or raises
        with self.ema.applied(self.model):
            return self._evaluate_model()

    def _evaluate_model(self) -> Dict[str, float]:
        was_training = self.model.training
        if was_training:
            self.model.eval()
            self._say("Model is converted to eval mode.")
        container = {'img_bbox': [], 'img_bbox2d': []}
        synthetic = str(self.cfg.DATA.ROOT).startswith('synthetic')
        for test_data in DevicePrefetcher(self.test_loader, self.current_device):
            test_data = move_data_device(test_data, self.current_device)
            if synthetic:            # KITTI text export needs dataset metadata the synthetic set does not have
                res = self.model.batch_eval(test_data, get_vis_format=True)
                container['img_bbox'].extend(r['img_bbox'] for r in res)
                container['img_bbox2d'].extend(r['img_bbox2d'] for r in res)
            else:
                res = self.model.batch_eval(test_data)
                for field in ('img_bbox', 'img_bbox2d'):
                    container[field].extend(res[field])
        eval_dict = self.test_dataset.evaluate(container, eval_classes=['Pedestrian', 'Cyclist', 'Car'], verbose=self.is_main)
        if was_training:
            self.model.train()
            self._say("Model is converted to train mode.")
        return eval_dict

    @torch.no_grad()
    def visualize(self, output_dir: str, draw_items: List[str] = ('bev', '2d', '3d')):
        raise NotImplementedError("drawing (cv2) is outside the MI355X hot path; use the reference's utils/visualizer.py "
                                  "on the output of model.batch_eval(data, get_vis_format=True)")
