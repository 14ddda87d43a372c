"""`python infer_raw.py --target_hw H W <the arguments of test_raw.py>`: test_raw.py -- a trained checkpoint over a KITTI raw
drive -- with the network's resolution as an argument.

This file holds no second copy of the raw-drive entry point: it takes ``--target_hw H W`` off the command line, makes (H, W) what
``KITTIRawDataset(resize_hw=None)`` means (``KITTIRawDataset.default_resize_hw``) and runs test_raw.py's own ``main`` on the rest.
The dataset then puts Resize3D((H, W), interpolation='exact') first in its list: the frames are resampled on the device with
their other image work (mc_preprocess_augmented, flag 1024), the calibration is rescaled per frame, and ``scale_hw`` maps the
boxes of the label files back to each source frame.  Without the argument it is test_raw.py.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    # (behind the __main__ guard: the loader's workers come from a fork server and import this module again)
    ap = argparse.ArgumentParser('MonoCon Tester for KITTI Raw Dataset, at a chosen resolution', add_help=False,
                                 usage="infer_raw.py [--target_hw H W] <arguments of test_raw.py, listed below>")
    ap.add_argument('--target_hw', type=int, nargs=2, default=None, metavar=('H', 'W'),
                    help="Run the network at this resolution: the frames are resampled on the device (default: their own size)")
    args, rest = ap.parse_known_args()
    if '-h' in rest or '--help' in rest:
        ap.print_help()
        print()
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
