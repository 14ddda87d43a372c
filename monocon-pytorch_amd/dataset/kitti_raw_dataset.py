"""KITTI *raw* drives: a directory of frames plus one ``calib_cam_to_cam.txt`` (reference dataset/kitti_raw_dataset.py).

Same contract as the reference: ``KITTIRawDataset(image_dir, calib_file, img_extension='png')`` lists the frames in sorted
glob order, ``SimpleCalib.P2`` is the calibration's ``P_rect_02``, and ``dataset[i]`` is the reference's batch-of-one
``data_dict`` (Normalize(keep_origin=True), Pad(32), ToTensor, Convert_3D_to_4D) with ``img_metas`` {'idx', 'image_path',
'ori_shape' = the 3-tuple (H, W, 3)}.  Frames are decoded with PIL, as MonoConDataset.load_image does (a PNG is lossless:
the same RGB array as the reference's cv2.imread + BGR2RGB).

Batched mode (not in the reference): with ``device_image=True`` a sample is the raw uint8 frame zero-padded to the padded
size plus the parameters of ``mc_preprocess_augmented`` (transforms.DeferImage / DeferredImage with no augmentation, i.e.
flags 0: Normalize + Pad + ToTensor on the device, bit-identical to the host transforms); ``collate_fn`` stacks them and
``MonoConDetector.finish_batch`` finishes the batch.  Its metas carry ``sample_idx`` = the frame index and, unlike the
batch-of-one dict, a 2-tuple ``ori_shape`` (H, W) -- the form the KITTI conversion reads.
"""
import glob
import os
from typing import Any, Dict, List

import numpy as np
from torch.utils.data import Dataset

from dataset.monocon_dataset import IMG_MEAN, IMG_STD, MonoConDataset, _resize
from transforms import Compose, Convert_3D_to_4D, DeferImage, DeferredImage, Normalize, Pad, ToTensor
from utils.engine_utils import tprint


def default_raw_transforms(resize_hw=None):
    return _resize(resize_hw) + [Normalize(mean=IMG_MEAN, std=IMG_STD, keep_origin=True), Pad(size_divisor=32), ToTensor(), Convert_3D_to_4D()]


class SimpleCalib:
    """the calibration of a raw drive as the detector reads it: ``.P2`` (3, 4) float32 = ``P_rect_02``"""

    def __init__(self, calib_dict: Dict[str, Any]):
        self.P2 = calib_dict['P_rect_02']

    def rescale(self, scale_x: float = None, scale_y: float = None) -> None:
        """the projection of the frame resized by these factors (KITTICalibration.rescale on P2; Resize3D calls it)"""
        self.P2[0, [0, 2, 3]] *= 1.0 if scale_x is None else scale_x
        self.P2[1, [1, 2, 3]] *= 1.0 if scale_y is None else scale_y


class KITTIRawDataset(Dataset):
    # what ``resize_hw=None`` means: None = the frames keep their size.  A front end that builds its dataset elsewhere sets it
    # before that (infer_raw.py runs test_raw.py's main at a chosen resolution this way)
    default_resize_hw = None

    def __init__(self, image_dir: str, calib_file: str, img_extension: str = 'png', device_image: bool = False,
                 resize_hw=None):
        super().__init__()
        if resize_hw is None:
            resize_hw = type(self).default_resize_hw
        assert os.path.isdir(image_dir), "image_dir %r is not a directory" % (image_dir,)
        assert os.path.isfile(calib_file), "calib_file %r is not a file (calib_cam_to_cam.txt)" % (calib_file,)
        img_extension = img_extension.replace('.', '')
        self.image_dir = image_dir
        self.image_files = sorted(glob.glob(os.path.join(self.image_dir, '*.%s' % img_extension)))
        self.calib = SimpleCalib(self._parse_calib(calib_file))
        self.device_image = device_image
        self.resized = len(_resize(resize_hw)) > 0
        # resize_hw (H, W): the network's resolution (Resize3D(interpolation='exact') first: on the device in batched mode)
        self.transforms = Compose([DeferImage()] + _resize(resize_hw) + [DeferredImage(size_divisor=32)] if device_image else
                                  default_raw_transforms(resize_hw))
        tprint("Found %d images in '%s'." % (len(self.image_files), image_dir))

    def __len__(self) -> int:
        return len(self.image_files)

    def load_image(self, idx: int) -> np.ndarray:
        from PIL import Image
        with Image.open(self.image_files[idx]) as im:
            return np.asarray(im.convert('RGB'), dtype=np.uint8)

    def __getitem__(self, idx: int) -> Dict[str, Any]:
        img = self.load_image(idx)
        if self.device_image:
            metas = {'idx': idx, 'sample_idx': idx, 'image_path': self.image_files[idx], 'ori_shape': img.shape[:2]}
        else:
            metas = {'idx': idx, 'image_path': self.image_files[idx], 'ori_shape': img.shape}
        # (Resize3D rescales the sample's calibration in place: it gets its own copy of the drive's)
        calib = SimpleCalib({'P_rect_02': self.calib.P2.copy()}) if self.resized else self.calib
        return self.transforms({'img': img, 'img_metas': metas, 'calib': calib})

    @staticmethod
    def collate_fn(batched: List[Dict[str, Any]]) -> Dict[str, Any]:
        """device_image samples -> one batch: uint8 frames (B, Hp, Wp, 3), ``img_aug`` (B, 24), metas as lists, calib list"""
        return MonoConDataset.collate_fn(batched)

    @staticmethod
    def _parse_calib(file_path: str) -> Dict[str, Any]:
        """``key: values`` lines of calib_cam_to_cam.txt.  Keys starting S_, R_, P_ or T_ hold numbers: float32 arrays, the P_
        ones shaped 3 x 4; any other key (calib_time, K_, D_) keeps its text."""
        out = {}
        with open(file_path, 'r') as f:
            for line in f:
                if not line.strip():
                    continue
                key, text = line.rstrip('\n').split(': ', 1)
                if key[:2] in ('S_', 'R_', 'P_', 'T_'):
                    arr = np.array([float(v) for v in text.split()], dtype=np.float64).astype(np.float32)
                    out[key] = arr.reshape(3, 4) if key.startswith('P_') else arr
                else:
                    out[key] = text
        return out
