"""KITTI raw drives on the host: dataset/kitti_raw_dataset.py (calibration parsing, frame order, the batch-of-one sample
and the batched device_image sample), the packed-row builder of MonoConDetector.detect and the test_raw.py command line.
The device side (mc_kitti_format, detect, test_raw.py end to end) is tests/test_hip_kitti_format.py."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, load_golden

MINI = os.path.join(GOLDEN, "kitti_mini", "training")
FRAMES = ("000007", "000011")

# calib_cam_to_cam.txt of a raw drive (layout of the 2011_09_26 drives), P_rect_02 = the kitti_mini frame 000007's P2
RAW_CALIB = """calib_time: 09-Jan-2012 13:57:47
corner_dist: 9.950000e-02
S_00: 1.392000e+03 5.120000e+02
K_00: 9.842439e+02 0.000000e+00 6.900000e+02 0.000000e+00 9.808141e+02 2.331966e+02 0.000000e+00 0.000000e+00 1.000000e+00
D_00: -3.728755e-01 2.037299e-01 2.219027e-03 1.383707e-03 -7.233722e-02
R_00: 1.000000e+00 0.000000e+00 0.000000e+00 0.000000e+00 1.000000e+00 0.000000e+00 0.000000e+00 0.000000e+00 1.000000e+00
T_00: 2.573699e-16 -1.059758e-16 1.614870e-16
S_rect_00: 1.242000e+03 3.750000e+02
R_rect_00: 9.999239e-01 9.837760e-03 -7.445048e-03 -9.869795e-03 9.999421e-01 -4.278459e-03 7.402527e-03 4.351614e-03 9.999631e-01
P_rect_00: 7.215377e+02 0.000000e+00 6.095593e+02 0.000000e+00 0.000000e+00 7.215377e+02 1.728540e+02 0.000000e+00 0.000000e+00 0.000000e+00 1.000000e+00 0.000000e+00
S_02: 1.392000e+03 5.120000e+02
K_02: 9.597910e+02 0.000000e+00 6.960217e+02 0.000000e+00 9.569251e+02 2.241806e+02 0.000000e+00 0.000000e+00 1.000000e+00
D_02: -3.691481e-01 1.968681e-01 1.353473e-03 5.677587e-04 -6.770705e-02
R_02: 9.999758e-01 -5.267463e-03 -4.552439e-03 5.251945e-03 9.999804e-01 -3.413835e-03 4.570332e-03 3.389843e-03 9.999838e-01
T_02: 5.956621e-02 2.900141e-04 2.577209e-03
S_rect_02: 1.242000e+03 3.750000e+02
R_rect_02: 9.998817e-01 1.511453e-02 -2.841595e-03 -1.511724e-02 9.998853e-01 -9.338510e-04 2.827154e-03 9.766976e-04 9.999955e-01
P_rect_02: 7.215377e+02 0.000000e+00 6.095593e+02 4.485728e+01 0.000000e+00 7.215377e+02 1.728540e+02 2.163791e-01 0.000000e+00 0.000000e+00 1.000000e+00 2.745884e-03
"""


def make_raw_drive(root, n_frames=2, ext="png"):
    """a raw drive under ``root``: frames 0000000000.<ext>, ... (the kitti_mini PNGs in turn) and calib_cam_to_cam.txt"""
    img_dir = os.path.join(str(root), "image_02", "data")
    os.makedirs(img_dir, exist_ok=True)
    for i in range(n_frames):
        shutil.copy(os.path.join(MINI, "image_2", FRAMES[i % 2] + ".png"), os.path.join(img_dir, "%010d.%s" % (i, ext)))
    calib = os.path.join(str(root), "calib_cam_to_cam.txt")
    with open(calib, "w") as f:
        f.write(RAW_CALIB)
    return img_dir, calib


def test_parse_calib_raw_layout(tmp_path):
    from dataset.kitti_raw_dataset import KITTIRawDataset, SimpleCalib
    from utils.data_classes import KITTICalibration
    _, calib = make_raw_drive(tmp_path, 0)
    d = KITTIRawDataset._parse_calib(calib)
    keys = [ln.split(":")[0] for ln in RAW_CALIB.strip().splitlines()]
    assert list(d) == keys
    for k, v in d.items():
        if k[:2] in ("S_", "R_", "P_", "T_"):
            assert isinstance(v, np.ndarray) and v.dtype == np.float32, k
            expect = {"S_": (2,), "R_": (9,), "T_": (3,), "P_": (3, 4)}[k[:2]]
            assert v.shape == expect, (k, v.shape)
        else:
            assert isinstance(v, str), k           # calib_time, corner_dist, K_xx, D_xx keep their text
    assert d["calib_time"] == "09-Jan-2012 13:57:47"
    P2 = SimpleCalib(d).P2
    ref = KITTICalibration(os.path.join(MINI, "calib", "000007.txt")).P2
    assert P2.dtype == np.float32 and P2.shape == (3, 4)
    assert P2.tobytes() == ref.tobytes()


def test_frame_order_and_extension(tmp_path):
    from dataset.kitti_raw_dataset import KITTIRawDataset
    img_dir, calib = make_raw_drive(tmp_path, 0)
    for name in ("0000000002.png", "0000000000.png", "0000000010.png", "0000000001.jpg", "notes.txt"):
        open(os.path.join(img_dir, name), "wb").close()
    ds = KITTIRawDataset(img_dir, calib)
    assert [os.path.basename(f) for f in ds.image_files] == ["0000000000.png", "0000000002.png", "0000000010.png"]
    assert len(ds) == 3
    for ext in ("jpg", ".jpg"):
        assert [os.path.basename(f) for f in KITTIRawDataset(img_dir, calib, img_extension=ext).image_files] == ["0000000001.jpg"]


def test_missing_paths_raise(tmp_path):
    from dataset.kitti_raw_dataset import KITTIRawDataset
    img_dir, calib = make_raw_drive(tmp_path, 1)
    with pytest.raises(AssertionError):
        KITTIRawDataset(os.path.join(str(tmp_path), "no_such_dir"), calib)
    with pytest.raises(AssertionError):
        KITTIRawDataset(img_dir, os.path.join(str(tmp_path), "no_such_calib.txt"))
    with pytest.raises(AssertionError):
        KITTIRawDataset(img_dir, img_dir)                  # a directory is not a calibration file


def _host_frame(path):
    """the test-list host transforms of MonoConDataset (Normalize, Pad, ToTensor) on the PIL-decoded frame"""
    from PIL import Image
    from dataset.monocon_dataset import default_transforms
    from transforms import Compose
    with Image.open(path) as im:
        arr = np.asarray(im.convert("RGB"), dtype=np.uint8)
    out = Compose(default_transforms())({"img": arr, "img_metas": {}})
    return arr, out["img"]


def test_getitem_is_the_reference_batch_of_one(tmp_path):
    from dataset.kitti_raw_dataset import KITTIRawDataset, SimpleCalib
    img_dir, calib = make_raw_drive(tmp_path, 2)
    ds = KITTIRawDataset(img_dir, calib)
    for i in range(2):
        d = ds[i]
        arr, ref = _host_frame(ds.image_files[i])
        assert tuple(d["img"].shape) == (1, 3, 384, 1248) and d["img"].dtype == torch.float32
        assert torch.equal(d["img"][0], ref)
        assert d["img_metas"] == {"idx": [i], "image_path": [ds.image_files[i]], "ori_shape": [arr.shape],
                                  "pad_shape": [(384, 1248)]}
        assert len(d["img_metas"]["ori_shape"][0]) == 3             # the reference keeps img.shape
        assert np.array_equal(d["ori_img"], arr.astype(np.float32))
        assert isinstance(d["calib"], list) and len(d["calib"]) == 1 and isinstance(d["calib"][0], SimpleCalib)


def test_device_image_batch(tmp_path):
    """device_image=True + collate_fn: uint8 frames zero-padded to 384x1248, mc_preprocess_augmented parameters with no
    augmentation flag, metas with sample_idx = frame index and (H, W) ori_shape"""
    from dataset.kitti_raw_dataset import KITTIRawDataset
    img_dir, calib = make_raw_drive(tmp_path, 3)
    ds = KITTIRawDataset(img_dir, calib, device_image=True)
    b = KITTIRawDataset.collate_fn([ds[i] for i in range(3)])
    assert tuple(b["img"].shape) == (3, 384, 1248, 3) and b["img"].dtype == torch.uint8
    assert tuple(b["img_aug"].shape) == (3, 24)
    assert b["img_aug"][:, 2].eq(0).all()                            # flags 0: Normalize + Pad + ToTensor only
    assert b["img_metas"]["sample_idx"] == [0, 1, 2] and b["img_metas"]["idx"] == [0, 1, 2]
    assert b["img_metas"]["pad_shape"] == [(384, 1248)] * 3
    for i in range(3):
        arr, _ = _host_frame(ds.image_files[i])
        h, w = arr.shape[:2]
        assert b["img_metas"]["ori_shape"][i] == (h, w)
        assert tuple(b["img_aug"][i, :2].tolist()) == (h, w)
        assert torch.equal(b["img"][i, :h, :w], torch.from_numpy(arr.copy()))
        assert int(b["img"][i, h:].sum()) == 0 and int(b["img"][i, :, w:].sum()) == 0
    assert all(c is ds.calib for c in b["calib"])


def _golden_annos():
    from hipmonocon import synth
    from utils.kitti_convert_utils import convert_to_kitti_2d, convert_to_kitti_3d
    g = load_golden("decode_k30.npz")
    metas = {"ori_shape": [(375, 1242)] * 4, "sample_idx": [11, 12, 13, 14]}
    res3d, res2d = [], []
    for i in range(4):
        b2, b3, lab = g["box2d.%d" % i], g["box3d.%d" % i], g["label.%d" % i]
        res3d.append({"boxes_3d": torch.from_numpy(b3), "scores_3d": torch.from_numpy(b2[:, 4]), "labels_3d": torch.from_numpy(lab)})
        res2d.append([b2[lab == c] for c in range(3)])
    return convert_to_kitti_3d(res3d, metas, [synth.SynthCalib() for _ in range(4)]), convert_to_kitti_2d(res2d, metas)


def test_annos_from_rows_rebuilds_the_host_conversion():
    """kitti_annos_from_rows (detect's builder) on rows packed from the host conversion of the reference decode: the same
    names, values, dtypes and sample_idx, including the images without a row"""
    from utils.kitti_convert_utils import CLASSES, _empty_anno, kitti_annos_from_rows
    k3, k2 = _golden_annos()
    k3.append(_empty_anno())                                      # an image without boxes, as the conversion leaves it
    k2.append(_empty_anno())
    B, K = 5, 40
    rows3d = np.full((B, K, 14), np.nan, np.float32)
    rows2d = np.full((B, K, 6), np.nan, np.float32)
    n3d, n2d = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for i in range(B):
        a = k3[i]
        n3d[i] = len(a["name"])
        rows3d[i, :n3d[i]] = np.column_stack([[CLASSES.index(s) for s in a["name"]], a["alpha"], a["bbox"], a["dimensions"],
                                              a["location"], a["rotation_y"], a["score"]]) if n3d[i] else 0
        a = k2[i]
        n2d[i] = len(a["name"])
        rows2d[i, :n2d[i]] = np.column_stack([[CLASSES.index(s) for s in a["name"]], a["bbox"], a["score"]]) if n2d[i] else 0
    sample_idx = [11, 12, 13, 14, 15]
    got = kitti_annos_from_rows(rows3d, n3d, rows2d, n2d, sample_idx)
    for field, ref in (("img_bbox", k3), ("img_bbox2d", k2)):
        assert len(got[field]) == B
        for i in range(B):
            a, r = got[field][i], ref[i]
            assert set(a) == set(r) | {"sample_idx"}
            assert list(a["name"]) == list(r["name"])
            for k in ("truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score"):
                assert a[k].shape == np.asarray(r[k]).shape, (field, i, k)
                assert a[k].dtype.kind == np.asarray(r[k]).dtype.kind, (field, i, k)
                assert np.allclose(a[k], np.asarray(r[k], np.float64), rtol=1e-6, atol=1e-5), (field, i, k)
            assert a["sample_idx"].tolist() == [sample_idx[i]] * len(r["name"])


def test_result_lines_are_the_submission_format(tmp_path):
    """the shared line helper writes what MonoConDataset.write_kitti_results writes"""
    from utils.kitti_convert_utils import kitti_result_lines
    k3, _ = _golden_annos()
    a = k3[0]
    lines = kitti_result_lines(a)
    assert len(lines) == len(a["name"]) > 0
    for ln, i in zip(lines, range(len(lines))):
        f = ln.split()
        assert f[0] == a["name"][i] and f[1:3] == ["-1", "-1"] and len(f) == 16 and ln.endswith("\n")
        bb, dm, lc = a["bbox"][i], a["dimensions"][i], a["location"][i]
        want = [a["alpha"][i], *bb, dm[1], dm[2], dm[0], *lc, a["rotation_y"][i], a["score"][i]]
        assert f[3:] == ["%.4f" % v for v in want]


def test_test_raw_cli_lists_the_reference_arguments():
    r = subprocess.run([sys.executable, os.path.join(PKG, "test_raw.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--data_dir", "--calib_file", "--checkpoint_file", "--gpu_id", "--save_dir", "--fps", "--batch_size",
                 "--num_workers", "--test_thres"):
        assert flag in r.stdout, flag
