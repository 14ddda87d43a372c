"""MonoConDetector: DLA-34 -> DLAUp -> MonoCon dense heads on MI355X.

Same constructor, attributes (``backbone``, ``neck``, ``head``), ``forward`` / ``batch_eval`` /
``load_checkpoint`` and state_dict keys as reference model/detector/monocon_detector.py:28-87.
In eval mode one ``mc_forward_infer`` call runs the whole NHWC plan (no NCHW round trips
between stages, no torch.cat); the ten prediction maps come back NCHW as the reference's.
"""
from typing import Any, Dict, Tuple

import torch
import torch.nn as nn

from hipmonocon.params import HipRuntime
from model.backbone import DLA, DLAUp
from model.dense_heads import MonoConDenseHeads

default_head_config = {'num_classes': 3, 'num_kpts': 9, 'num_alpha_bins': 12, 'max_objs': 30}
default_test_config = {'topk': 30, 'local_maximum_kernel': 3, 'max_per_img': 30, 'test_thres': 0.4}


class MonoConDetector(nn.Module):
    def __init__(self, num_dla_layers: int = 34, pretrained_backbone: bool = True,
                 head_config: Dict[str, Any] = None, test_config: Dict[str, Any] = None):
        super().__init__()
        self.backbone = DLA(num_dla_layers, pretrained=pretrained_backbone)
        self.neck = DLAUp(self.backbone.get_out_channels(start_level=2), start_level=2)
        if head_config is None:
            head_config = default_head_config
        if test_config is None:
            test_config = default_test_config
        self.head = MonoConDenseHeads(in_ch=64, test_config=test_config, **head_config)
        self._rt = HipRuntime()

    def set_precision(self, mode: str = "fp32"):
        """Arithmetic of the convolutions.  'fp32' (default): the fp32 matrix pipe.  'bf16x3' / 'f16x2': fp32 values
        emulated on the bf16 / fp16 matrix pipe by a 3-way / 2-way operand split (same parity tolerances as 'fp32').
        'bf16': bf16 MFMA operands with fp32 accumulation, activations, master weights, BN statistics and losses
        (no reference counterpart, not within the parity tolerance)."""
        self._rt.set_precision(mode)
        return self

    def _engine(self):
        return self._rt.get(self.state_dict(keep_vars=True))

    def finish_batch(self, data_dict: Dict[str, Any]) -> Dict[str, Any]:
        """a collated batch of transforms.DeferredImage samples -- raw uint8 frames (B, Hp, Wp, 3) + ``img_aug`` (B, 24) -- gets
        its float32 (B, 3, Hp, Wp) frames here, in one launch (mc_preprocess_augmented: the train augmentations' image work +
        Normalize + Pad + ToTensor, bit-identical to the host transforms), at the size ``img_metas['pad_shape']`` names: the
        canvas's, or that of a deferred Resize3D's target.  Any other batch passes through."""
        if 'img_aug' in data_dict:
            eng = self._rt.engine if self._rt.engine is not None else self._engine()
            from dataset.monocon_dataset import IMG_MEAN, IMG_STD
            from hipmonocon.lib import MonoconHipError
            # the output's size: what Pad made of the frame the network sees -- the canvas's own size unless a deferred
            # Resize3D resamples the frames on the way
            out_hw = None
            pads = data_dict.get('img_metas', {}).get('pad_shape')
            if pads is not None:
                pads = {(int(p[0]), int(p[1])) for p in (pads if isinstance(pads, list) else [pads])}
                if len(pads) != 1:
                    raise MonoconHipError("finish_batch: the batch disagrees on pad_shape: %s" % sorted(pads))
                out_hw = pads.pop()
            data_dict['img'] = eng.preprocess_augmented(data_dict['img'].contiguous(), data_dict.pop('img_aug').contiguous(),
                                                        IMG_MEAN, IMG_STD, out_hw=out_hw)
        return data_dict

    def forward(self, data_dict: Dict[str, Any], return_loss: bool = True) -> Tuple[Dict[str, torch.Tensor]]:
        img = self.finish_batch(data_dict)['img']
        if self.training:
            from hipmonocon.train import forward_train
            pred_dict, loss_dict = forward_train(self, data_dict)
            return (pred_dict, loss_dict) if return_loss else pred_dict
        return self._engine().forward_infer(img.contiguous())

    def batch_eval(self, data_dict: Dict[str, Any], get_vis_format: bool = False) -> Dict[str, Any]:
        if self.training:
            raise Exception("Model is in training mode. Please use '.eval()' first.")
        pred_dict = self.forward(data_dict, return_loss=False)
        return self.head._get_eval_formats(data_dict, pred_dict, get_vis_format=get_vis_format,
                                           engine=self._rt.engine)

    def detect(self, data_dict: Dict[str, Any], get_vis_format: bool = False):
        """what ``batch_eval`` returns -- the KITTI annotation dicts {'img_bbox': [...], 'img_bbox2d': [...]} with
        ``sample_idx``, or the visualiser's list (get_vis_format=True) -- with the per-image host tail moved to the device:
        forward, mc_decode, mc_nms3d when test_config['nms_thres'] is set, mc_kitti_format (the KITTI rows of the whole batch in
        one launch), then ONE copy to page-locked
        host memory and one wait for it.  The annotation dicts are built from the packed rows (utils/kitti_convert_utils.py
        kitti_annos_from_rows); the visualiser's list from the decode's outputs (it wants every kept box, visible or not)."""
        kitti, vis = self._detect(data_dict, want_kitti=not get_vis_format, want_vis=bool(get_vis_format))
        return vis if get_vis_format else kitti

    def detect_with_vis(self, data_dict: Dict[str, Any]):
        """(annotation dicts, visualiser's list) of ``detect`` from one forward"""
        return self._detect(data_dict, want_kitti=True, want_vis=True)

    def _pinned(self, name: str, n: int, dtype) -> torch.Tensor:
        """a page-locked host buffer of this detector, grown on demand (callers wait for the copies that use it)"""
        pins = self.__dict__.setdefault('_pins', {})
        buf = pins.get(name)
        if buf is None or buf.numel() < n:
            buf = pins[name] = torch.empty(n, dtype=dtype, pin_memory=True)
        return buf[:n]

    def _detect(self, data_dict: Dict[str, Any], want_kitti: bool, want_vis: bool):
        if self.training:
            raise Exception("Model is in training mode. Please use '.eval()' first.")
        import numpy as np
        from hipmonocon.engine import p2_inverse
        from utils.kitti_convert_utils import img_hw_scale, kitti_annos_from_rows
        img = self.finish_batch(data_dict)['img']
        B, dev = int(img.shape[0]), img.device
        metas = data_dict['img_metas']
        calib = data_dict['calib'] if isinstance(data_dict['calib'], (list, tuple)) else [data_dict['calib']] * B
        # P2, its inverse and the per-image (ori_h, ori_w, inv_sx, inv_sy) rows go up in one asynchronous copy, queued
        # before the forward
        P2 = np.stack([np.asarray(c.P2, dtype=np.float32).reshape(3, 4) for c in calib])
        inp = np.concatenate([P2.reshape(-1), p2_inverse(P2).reshape(-1), img_hw_scale(metas, B).reshape(-1)])
        host_in = self._pinned('in', inp.size, torch.float32)
        host_in.numpy()[:] = inp
        dev_in = host_in.to(dev, non_blocking=True)
        P2_d, P2inv_d, hws_d = dev_in[:12 * B].view(B, 3, 4), dev_in[12 * B:28 * B].view(B, 4, 4), dev_in[28 * B:].view(B, 4)

        eng = self._engine()
        pred_dict = eng.forward_infer(img.contiguous())
        R = self.head._decode_dense(data_dict, pred_dict, eng, calib_dev=(P2_d, P2inv_d))
        K = int(R['box2d'].shape[1])
        parts = []                                  # device tensors -> byte ranges of one page-locked buffer
        if want_vis:                                # the mask of the boxes to ship: after NMS when test_config turns it on
            parts += [R['cls'], R['box2d'], R['box3d'], R['keep_nms'] if 'keep_nms' in R else R['keep_thr']]
        if want_kitti:
            parts.insert(0, eng.kitti_format(R, P2_d, hws_d)['packed'])
        nbytes = [t.numel() * t.element_size() for t in parts]
        host = self._pinned('out', sum(nbytes), torch.uint8)
        off = 0
        for t, n in zip(parts, nbytes):
            host[off:off + n].copy_(t.reshape(-1).view(torch.uint8), non_blocking=True)
            off += n
        done = torch.cuda.Event()
        done.record()
        done.synchronize()

        hb, off = host.numpy(), 0
        kitti = vis = None
        if want_kitti:
            f = hb[:nbytes[0]].view(np.float32)
            counts = f[B * K * 20:].view(np.int32)
            sample_idx = metas['sample_idx'] if 'sample_idx' in metas else metas.get('idx', list(range(B)))
            kitti = kitti_annos_from_rows(f[:B * K * 14].reshape(B, K, 14), counts[:B], f[B * K * 14:B * K * 20].reshape(B, K, 6),
                                          counts[B:], sample_idx)
            off = nbytes[0]
        if want_vis:
            cls = hb[off:off + B * K * 8].view(np.int64).reshape(B, K)
            off += B * K * 8
            box2d = hb[off:off + B * K * 20].view(np.float32).reshape(B, K, 5)
            off += B * K * 20
            box3d = hb[off:off + B * K * 28].view(np.float32).reshape(B, K, 7)
            off += B * K * 28
            keep = hb[off:off + B * K].reshape(B, K).astype(bool)
            nc = self.head.num_classes
            vis = []
            for i in range(B):
                b2, b3, lab = box2d[i][keep[i]], box3d[i][keep[i]], cls[i][keep[i]]
                per_class = ([b2[lab == c] for c in range(nc)] if len(b2) else
                             [np.zeros((0, 5), dtype=np.float32) for _ in range(nc)])
                vis.append({'img_bbox': dict(boxes_3d=torch.from_numpy(b3), scores_3d=torch.from_numpy(b2[:, -1].copy()),
                                             labels_3d=torch.from_numpy(lab)),
                            'img_bbox2d': per_class})
        return kitti, vis

    def load_checkpoint(self, ckpt_file: str, use_ema: bool = False):
        """``use_ema``: the checkpoint's averaged weights (written by a run with SOLVER.EMA.ENABLE, solver/model_ema.py)
        instead of the live ones; a file without them is an error, never a silent use of the live weights"""
        # the reference pickles whole engine objects; torch >= 2.6 needs weights_only=False for those
        from utils.engine_utils import load_checkpoint_file
        state = load_checkpoint_file(ckpt_file)['state_dict']
        if use_ema:
            if state.get('ema') is None:
                raise KeyError("checkpoint '%s' holds no averaged weights (state_dict['ema']): it was written without "
                               "SOLVER.EMA.ENABLE; run without --use_ema to use its live weights" % ckpt_file)
            model_dict = state['ema']['tensors']
        else:
            model_dict = state['model']
        self.load_state_dict(model_dict)

    def _extract_feat_from_data_dict(self, data_dict: Dict[str, Any]) -> torch.Tensor:
        _, feat = self._engine().forward_infer(self.finish_batch(data_dict)['img'].contiguous(), want_feat=True)
        return feat
