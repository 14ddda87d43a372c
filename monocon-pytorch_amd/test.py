"""`python test.py --config_file cfg.yaml --checkpoint_file x.pth [--evaluate]` (reference test.py:12-70)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from engine.monocon_engine import MonoconEngine        # noqa: E402
from utils.engine_utils import load_cfg, tprint         # noqa: E402


def main():
    # (behind the __main__ guard: the loaders' workers come from a fork server and import this module again)
    ap = argparse.ArgumentParser('MonoCon Tester for KITTI 3D Object Detection Dataset')
    ap.add_argument('--config_file', type=str, required=True)
    ap.add_argument('--checkpoint_file', type=str, required=True)
    ap.add_argument('--gpu_id', type=int, default=0)
    ap.add_argument('--evaluate', action='store_true')
    ap.add_argument('--nms_thres', type=float, default=None,
                    help="IoU threshold of the opt-in 3D-box NMS after the decode (default: off, as the reference)")
    ap.add_argument('--nms_mode', type=str, default='bev', choices=('bev', '3d'),
                    help="Overlap of the NMS: rotated bird's-eye-view IoU or 3D IoU")
    ap.add_argument('--nms_class_agnostic', action='store_true', help="Let boxes of different classes suppress each other")
    ap.add_argument('--use_ema', action='store_true',
                    help="Evaluate the checkpoint's averaged weights (a run with SOLVER.EMA.ENABLE) instead of the live ones")
    args = ap.parse_args()

    cfg = load_cfg(args.config_file)
    cfg.GPU_ID = args.gpu_id
    engine = MonoconEngine(cfg, auto_resume=False, is_test=True)
    engine.load_checkpoint(args.checkpoint_file, verbose=True)
    if args.use_ema:
        engine.model.load_checkpoint(args.checkpoint_file, use_ema=True)    # (raises if the file has none)
        tprint("Averaged (EMA) weights of '%s' are loaded to model." % args.checkpoint_file)
    if args.nms_thres is not None:
        # the head reads these keys when it decodes; a copy, so that the detector's default dict stays as it is
        engine.model.head.test_config = dict(engine.model.head.test_config, nms_thres=args.nms_thres, nms_mode=args.nms_mode,
                                             nms_class_agnostic=args.nms_class_agnostic)
    if args.evaluate:
        tprint("Mode: Evaluation")
        print(engine.evaluate())


if __name__ == '__main__':
    main()
