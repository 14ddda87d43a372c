"""`python test_raw.py --data_dir <frames> --calib_file calib_cam_to_cam.txt --checkpoint_file x.pth --save_dir out`
(reference test_raw.py): a trained checkpoint over a KITTI raw drive.

Frames are read in batches by loader workers and finished on the device (KITTIRawDataset(device_image=True) +
mc_preprocess_augmented); MonoConDetector.detect_with_vis runs forward, decode and the KITTI formatting of the batch on the
device.  Writes one KITTI label file per frame, ``<save_dir>/<frame stem>.txt``, and ``<save_dir>/vis_results.pt``: the list
the reference hands to its Visualizer.  The drawing and the video export themselves are out of scope (no cv2 here).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    # (behind the __main__ guard: the loader's workers come from a fork server and import this module again)
    import torch
    from torch.utils.data import DataLoader

    from dataset.kitti_raw_dataset import KITTIRawDataset
    from hipmonocon.feed import WORKER_CONTEXT, prepare_worker_context
    from model.detector import MonoConDetector
    from model.detector.monocon_detector import default_test_config
    from utils.engine_utils import move_data_device, tprint
    from utils.kitti_convert_utils import kitti_result_lines

    ap = argparse.ArgumentParser('MonoCon Tester for KITTI Raw Dataset')
    ap.add_argument('--data_dir', type=str, help="Path where sequence images are saved")
    ap.add_argument('--calib_file', type=str, help="Path to calibration file (.txt)")
    ap.add_argument('--checkpoint_file', type=str, help="Path of the checkpoint file (.pth)")
    ap.add_argument('--gpu_id', type=int, default=0, help="Index of GPU to use for testing")
    ap.add_argument('--fps', type=int, default=25, help="FPS of the result video (accepted; video export is not built)")
    ap.add_argument('--save_dir', type=str, help="Directory for the label files and vis_results.pt")
    ap.add_argument('--batch_size', type=int, default=16, help="Frames per forward")
    ap.add_argument('--num_workers', type=int, default=4, help="Loader workers decoding frames")
    ap.add_argument('--test_thres', type=float, default=None,
                    help="Score threshold of the decode (default: the detector's test_config, %s)" % default_test_config['test_thres'])
    args = ap.parse_args()

    tprint("Note: --fps=%d is ignored: drawing and video export are out of scope; vis_results.pt holds the visualiser's input."
           % args.fps)
    os.makedirs(args.save_dir, exist_ok=True)
    dataset = KITTIRawDataset(args.data_dir, args.calib_file, device_image=True)

    torch.cuda.set_device(args.gpu_id)
    device = 'cuda:%d' % args.gpu_id
    test_config = dict(default_test_config)
    if args.test_thres is not None:
        test_config['test_thres'] = args.test_thres
    detector = MonoConDetector(pretrained_backbone=False, test_config=test_config)
    detector.load_checkpoint(args.checkpoint_file)
    detector.to(device)
    detector.eval()
    tprint("Checkpoint '%s' is loaded to model." % args.checkpoint_file)

    if args.num_workers > 0:
        prepare_worker_context()
    loader = DataLoader(dataset, batch_size=args.batch_size, shuffle=False, num_workers=args.num_workers,
                        collate_fn=KITTIRawDataset.collate_fn, pin_memory=True,
                        multiprocessing_context=WORKER_CONTEXT if args.num_workers > 0 else None)
    vis_results = []
    t0 = time.perf_counter()
    with torch.no_grad():
        for data in loader:
            data = move_data_device(data, device)
            kitti, vis = detector.detect_with_vis(data)
            for path, anno in zip(data['img_metas']['image_path'], kitti['img_bbox']):
                stem = os.path.splitext(os.path.basename(path))[0]
                with open(os.path.join(args.save_dir, stem + '.txt'), 'w') as f:
                    f.writelines(kitti_result_lines(anno))
            vis_results.extend(vis)
    sec = time.perf_counter() - t0
    torch.save(vis_results, os.path.join(args.save_dir, 'vis_results.pt'))
    tprint("%d frames in %.2f s (%.1f frames/s): label files and vis_results.pt written to '%s'."
           % (len(vis_results), sec, len(vis_results) / max(sec, 1e-9), args.save_dir))


if __name__ == '__main__':
    main()
