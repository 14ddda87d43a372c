"""`python infer_raw.py --target_hw H W <the arguments of test_raw.py>`: test_raw.py -- a trained checkpoint over a KITTI raw
drive -- with the network's resolution as an argument.

This file holds no second copy of the raw-drive entry point: it takes ``--target_hw H W`` off the command line, makes (H, W) what
``KITTIRawDataset(resize_hw=None)`` means (``KITTIRawDataset.default_resize_hw``) and runs test_raw.py's own ``main`` on the rest.
The dataset then puts Resize3D((H, W), interpolation='exact') first in its list: the frames are resampled on the device with
their other image work (mc_preprocess_augmented, flag 1024), the calibration is rescaled per frame, and ``scale_hw`` maps the
boxes of the label files back to each source frame.  Without the argument it is test_raw.py.

``--nms_thres T [--nms_mode bev|3d] [--nms_class_agnostic]`` turn on the 3D-box NMS after the decode (mc_nms3d; off by
default, the reference has none): taken off the command line and added to the test_config that test_raw.py builds, by the
detector class its ``main`` finds in ``model.detector``.  Nothing outside this script's process and nothing in the package
changes for it.

``--use_ema`` runs the drive on the checkpoint's averaged weights (``state_dict['ema']``, written by a run with
SOLVER.EMA.ENABLE; solver/model_ema.py) instead of the live ones, the same way: the detector class test_raw.py finds loads
them in its ``load_checkpoint``, and a file without an average is an error, not a silent use of the live weights.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    # (behind the __main__ guard: the loader's workers come from a fork server and import this module again)
    ap = argparse.ArgumentParser('MonoCon Tester for KITTI Raw Dataset, at a chosen resolution', add_help=False,
                                 usage="infer_raw.py [--target_hw H W] [--nms_thres T [--nms_mode M] [--nms_class_agnostic]] [--use_ema] <arguments of test_raw.py, listed below>")
    ap.add_argument('--target_hw', type=int, nargs=2, default=None, metavar=('H', 'W'),
                    help="Run the network at this resolution: the frames are resampled on the device (default: their own size)")
    ap.add_argument('--nms_thres', type=float, default=None,
                    help="IoU threshold of the opt-in 3D-box NMS after the decode (default: off, as the reference)")
    ap.add_argument('--nms_mode', type=str, default='bev', choices=('bev', '3d'),
                    help="Overlap of the NMS: rotated bird's-eye-view IoU or 3D IoU")
    ap.add_argument('--nms_class_agnostic', action='store_true', help="Let boxes of different classes suppress each other")
    ap.add_argument('--use_ema', action='store_true',
                    help="Use the checkpoint's averaged weights (a run with SOLVER.EMA.ENABLE) instead of the live ones")
    args, rest = ap.parse_known_args()
    if '-h' in rest or '--help' in rest:
        ap.print_help()
        print()
    if args.nms_thres is not None:
        # test_raw.py builds its own test_config and detector: it looks the class up in model.detector when its main runs,
        # and finds one there whose constructor adds the three keys to the test_config it is given
        import model.detector as detector_pkg
        from model.detector.monocon_detector import default_test_config
        nms_keys = dict(nms_thres=args.nms_thres, nms_mode=args.nms_mode, nms_class_agnostic=args.nms_class_agnostic)

        class MonoConDetectorWithNms(detector_pkg.MonoConDetector):
            def __init__(self, *a, test_config=None, **kw):
                super().__init__(*a, test_config=dict(default_test_config if test_config is None else test_config, **nms_keys),
                                 **kw)

        detector_pkg.MonoConDetector = MonoConDetectorWithNms
    if args.use_ema:
        # (after the NMS class, so that both can be asked for: this one derives from whatever model.detector holds now)
        import model.detector as detector_pkg

        class MonoConDetectorWithEma(detector_pkg.MonoConDetector):
            def load_checkpoint(self, ckpt_file, use_ema=True):
                super().load_checkpoint(ckpt_file, use_ema=True)        # (raises if the file holds no average)

        detector_pkg.MonoConDetector = MonoConDetectorWithEma
    if args.target_hw is not None:
        if min(args.target_hw) < 1:
            ap.error("--target_hw needs two positive integers")
        from dataset.kitti_raw_dataset import KITTIRawDataset
        KITTIRawDataset.default_resize_hw = tuple(args.target_hw)
    import test_raw
    sys.argv = [sys.argv[0]] + rest
    test_raw.main()


if __name__ == '__main__':
    main()
