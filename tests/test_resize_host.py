"""Resize3D on the device path, host side: the resample both sides share (`transforms.resize_bilinear_u8`: float32 operation by
operation, the specification in include/monocon_hip.h), `Resize3D(interpolation='exact')` on the host and deferred behind
DeferImage, the parameter row DeferredImage writes for it (flag 1024, slots 0-1 the resized size, 17-18 the frame's own), and
the public switches (`resize_hw=` of the transform lists and datasets, config `DATA.RESIZE_HW`).  tests/test_resize_device.py
holds the kernel against what is pinned here."""
import copy
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MINI = os.path.join(GOLDEN, "kitti_mini")
SRC_HW, TARGET_HW, CROP_HW = (75, 131), (64, 96), (48, 64)
ALL_STAGES = 1024 | 1 | 128 | 256 | 512


def random_frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth_frame(h, w):
    """slow gradients and one sinusoid per channel: neighbouring taps differ by little, as in a photograph"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = [127.5 + 127.5 * np.sin(x / 37.0 + y / 53.0), 255.0 * x / (w - 1), 255.0 * (y / (h - 1)) * (1.0 - x / (w - 1))]
    return np.clip(np.rint(np.stack(ch, -1)), 0, 255).astype(np.uint8)


def sample(frame, seed=0):
    """an untransformed sample around ``frame``: the calibration of a kitti_mini frame and two labelled objects whose boxes
    cover most of the frame (so that shift and crop always keep one and record their operation)"""
    from utils.data_classes import KITTICalibration
    h, w = frame.shape[:2]
    m = 4
    rng = np.random.default_rng(1000 + seed)
    label = {'gt_bboxes': np.zeros((m, 4), np.float32), 'gt_labels': np.zeros(m, np.uint8),
             'gt_bboxes_3d': np.zeros((m, 7), np.float32), 'gt_labels_3d': np.zeros(m, np.uint8),
             'centers2d': np.zeros((m, 2), np.float32), 'depths': np.zeros(m, np.float32),
             'gt_kpts_2d': np.zeros((m, 18), np.float32), 'gt_kpts_valid_mask': np.zeros((m, 9), np.uint8),
             'mask': np.zeros((m,), np.bool_)}
    for row, box in enumerate(([0.08 * w, 0.1 * h, 0.93 * w, 0.9 * h], [0.3 * w, 0.25 * h, 0.8 * w, 0.85 * h])):
        label['gt_bboxes'][row] = box
        label['gt_labels'][row] = label['gt_labels_3d'][row] = row
        label['gt_bboxes_3d'][row] = rng.uniform(1, 20, 7)
        label['centers2d'][row] = [(box[0] + box[2]) / 2, (box[1] + box[3]) / 2]
        label['depths'][row] = 10 + row
        label['gt_kpts_2d'][row] = rng.uniform(0, 1, 18) * np.tile([w, h], 9)
        label['gt_kpts_valid_mask'][row] = 2
        label['mask'][row] = True
    return {'img': frame.copy(), 'label': label, 'calib': KITTICalibration(os.path.join(MINI, "training", "calib", "000007.txt")),
            'img_metas': {'idx': seed, 'sample_idx': seed, 'ori_shape': (h, w)}}


def train_list(seed, device_image, target_hw=TARGET_HW, crop_hw=CROP_HW):
    """the train list behind Resize3D('exact') with shift, flip and crop certain to fire (the colour stage always runs; which of
    its operations are drawn depends on the seed)"""
    import transforms as T
    from dataset.monocon_dataset import IMG_MEAN, IMG_STD
    rng = np.random.default_rng(seed)
    aug = [T.Resize3D(target_hw, interpolation='exact'),
           T.PhotometricDistortion(brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18, rng=rng),
           T.RandomShift(prob=1.0, shift_range=(-12, 12), hide_kpts_in_shift_area=True, rng=rng),
           T.RandomHorizontalFlip(prob=1.0, rng=rng),
           T.RandomCrop3D(prob=1.0, crop_size=crop_hw, hide_kpts_in_crop_area=True, rng=rng)]
    if device_image:
        return T.Compose([T.DeferImage()] + aug + [T.DeferredImage(size_divisor=32)])
    return T.Compose(aug + [T.Normalize(mean=IMG_MEAN, std=IMG_STD), T.Pad(size_divisor=32), T.ToTensor()])


def host_and_deferred(seed, src_hw=SRC_HW):
    frame = random_frame(src_hw[0], src_hw[1], 50 + seed)
    return train_list(seed, False)(sample(frame, seed)), train_list(seed, True)(sample(frame, seed)), frame


def metas_equal(a, b):
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def interpret(frame, prm):
    """what a parameter row says, carried out in numpy: the resample and the host transforms' own code, stage by stage in the
    kernel's order -> the float32 CHW image"""
    from dataset.monocon_dataset import IMG_MEAN, IMG_STD
    from transforms import default_transforms as T
    from transforms.augmentations import PhotometricDistortion, resize_bilinear_u8
    H, W, flags = int(prm[0]), int(prm[1]), int(prm[2])
    if flags & T.AUG_RESIZE:
        img = resize_bilinear_u8(frame[:int(prm[17]), :int(prm[18])].numpy(), (H, W))
    else:
        img = frame[:H, :W].numpy()
    if flags & T.AUG_COLOUR:
        p = {"brightness": prm[3] if flags & T.AUG_BRIGHTNESS else None, "contrast_before": prm[4] if flags & T.AUG_CONTRAST_BEFORE else None,
             "saturation": prm[5] if flags & T.AUG_SATURATION else None, "hue": prm[6] if flags & T.AUG_HUE else None,
             "contrast_after": prm[7] if flags & T.AUG_CONTRAST_AFTER else None,
             "permutation": prm[8:11].astype(np.int64) if flags & T.AUG_PERMUTATION else None}
        img = PhotometricDistortion.apply(img, p)
    if flags & T.AUG_SHIFT:
        sx, sy = int(prm[11]), int(prm[12])
        canvas = np.zeros_like(img)
        h, w = H - abs(sy), W - abs(sx)
        canvas[max(0, sy):max(0, sy) + h, max(0, sx):max(0, sx) + w] = img[max(0, -sy):max(0, -sy) + h, max(0, -sx):max(0, -sx) + w]
        img = canvas
    if flags & T.AUG_FLIP:
        img = img[:, ::-1, :]
    if flags & T.AUG_WINDOW:
        x0, y0, x1, y1 = (int(v) for v in prm[13:17])
        canvas = np.zeros_like(img)
        canvas[y0:y1, x0:x1] = img[y0:y1, x0:x1]
        img = canvas
    d = {"img": img, "img_metas": {}}
    for t in (T.Normalize(mean=IMG_MEAN, std=IMG_STD), T.Pad(32), T.ToTensor()):
        d = t(d)
    return d["img"]


# ------------------------------------------------------------------------------------------------ 1. against torch
@pytest.mark.parametrize("src_hw,target_hw", [((375, 1242), (288, 960)), ((370, 1224), (384, 1280))])
@pytest.mark.parametrize("kind", ["random", "smooth"])
def test_exact_resample_agrees_with_the_torch_resample(src_hw, target_hw, kind):
    """resize_bilinear_u8 against the default Resize3D (torch's bilinear interpolation): the same geometry, so after rounding to
    uint8 no value is more than one level apart and at most 1e-4 of the values differ at all (torch's float results depend on
    the vector path it takes on the host CPU: a condition of this test, not a tolerance of the device path)"""
    from transforms import Resize3D, resize_bilinear_u8
    frame = random_frame(*src_hw, seed=3) if kind == "random" else smooth_frame(*src_hw)
    got = resize_bilinear_u8(frame, target_hw)
    d = sample(frame)
    del d['label']
    want = Resize3D(target_hw)(d)['img']
    assert got.dtype == np.uint8 and got.shape == target_hw + (3,) and want.dtype == np.uint8
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print("resize %s %s -> %s: %d of %d values differ, max %d" % (kind, src_hw, target_hw, int((diff > 0).sum()), diff.size, int(diff.max())))
    assert int(diff.max()) <= 1
    assert int((diff > 0).sum()) <= 1e-4 * diff.size


# ------------------------------------------------------------------------------------------------ 2. exact cases
def test_exactly_representable_cases():
    from transforms import resize_bilinear_u8
    frame = random_frame(48, 80, seed=5)
    mean = frame.astype(np.float64).reshape(24, 2, 40, 2, 3).sum(axis=(1, 3)) / 4.0        # quarters: exact
    assert np.array_equal(resize_bilinear_u8(frame, (24, 40)), np.rint(mean).astype(np.uint8))     # np.rint: half to even
    assert (mean % 1 == 0.5).any()                                                        # (ties did occur)
    for hw in ((48, 80), (37, 61)):
        f = random_frame(*hw, seed=6)
        assert np.array_equal(resize_bilinear_u8(f, hw), f)
    with pytest.raises(TypeError):
        resize_bilinear_u8(frame.astype(np.float32), (24, 40))


# ------------------------------------------------------------------------------------------------ 3. deferred == host
def test_deferred_exact_resize_carries_the_host_transforms_bookkeeping():
    import transforms as T
    frame = random_frame(*SRC_HW, seed=7)
    th, tw = TARGET_HW
    host = T.Resize3D(TARGET_HW, interpolation='exact')(sample(frame))
    dev = T.Resize3D(TARGET_HW, interpolation='exact')(T.DeferImage()(sample(frame)))
    assert dev['img_ops'] == [('resize', (th, tw))]
    assert np.array_equal(dev['img'], frame) and np.array_equal(host['img'], T.resize_bilinear_u8(frame, TARGET_HW))
    for k in host['label']:
        assert np.array_equal(host['label'][k], dev['label'][k]), k
    for name in ('P0', 'P1', 'P2', 'P3'):
        assert np.array_equal(getattr(host['calib'], name), getattr(dev['calib'], name))
    metas_equal(host['img_metas'], dev['img_metas'])
    assert host['img_metas']['ori_shape'] == (th, tw)
    assert np.array_equal(host['img_metas']['scale_hw'], np.array([th / SRC_HW[0], tw / SRC_HW[1]]))
    untouched = sample(frame)
    assert np.allclose(host['label']['gt_bboxes'], untouched['label']['gt_bboxes'] * np.array([tw / 131, th / 75] * 2, np.float32))
    assert np.allclose(host['calib'].P2[0], untouched['calib'].P2[0] * tw / 131) and np.allclose(host['calib'].P2[1], untouched['calib'].P2[1] * th / 75)

    out = T.DeferredImage(size_divisor=32)(dev)
    prm = out['img_aug'].numpy()
    assert prm.dtype == np.float32 and prm.shape == (T.default_transforms.AUG_PARAMS,)
    assert (prm[0], prm[1], prm[2], prm[17], prm[18]) == (th, tw, T.default_transforms.AUG_RESIZE, SRC_HW[0], SRC_HW[1])
    assert T.default_transforms.AUG_RESIZE == 1024 and T.default_transforms._AUG_ORDER == ('resize', 'colour', 'shift', 'flip', 'window')
    assert not prm[3:17].any() and not prm[19:].any()
    assert out['img'].dtype == torch.uint8 and tuple(out['img'].shape) == (96, 160, 3)          # the SOURCE frame, padded to 32
    assert np.array_equal(out['img'][:75, :131].numpy(), frame)
    assert int(out['img'][75:].sum()) == 0 and int(out['img'][:, 131:].sum()) == 0
    assert out['img_metas']['pad_shape'] == (64, 96)                                          # Pad(32) of the TARGET
    host_padded = T.Pad(32)(T.Normalize([0, 0, 0], [1, 1, 1])(host))
    assert host_padded['img_metas']['pad_shape'] == out['img_metas']['pad_shape']
    assert 'img_ops' not in out


# ------------------------------------------------------------------------------------------------ 4. the row's meaning
def test_parameter_rows_reproduce_the_host_pipelines_image():
    """Resize3D('exact') -> PhotometricDistortion -> RandomShift -> RandomHorizontalFlip -> RandomCrop3D -> Normalize -> Pad ->
    ToTensor on the host against the deferred sample's row carried out by ``interpret``: the float32 images are bit-equal, and
    labels, calibration and metas agree (the flip mirrors about the RESIZED width although the deferred frame still has its own)"""
    seen = 0
    for seed in range(12):
        host, dev, frame = host_and_deferred(seed)
        prm = dev['img_aug'].numpy()
        flags = int(prm[2])
        assert flags & ALL_STAGES == ALL_STAGES, (seed, flags)
        assert (int(prm[0]), int(prm[1]), int(prm[17]), int(prm[18])) == TARGET_HW + SRC_HW
        assert np.array_equal(dev['img'][:SRC_HW[0], :SRC_HW[1]].numpy(), frame)
        for k in host['label']:
            assert torch.equal(host['label'][k], dev['label'][k]), (seed, k)
        assert np.array_equal(host['calib'].P2, dev['calib'].P2)
        metas_equal(host['img_metas'], dev['img_metas'])
        want = host['img']
        assert want.dtype == torch.float32 and tuple(want.shape) == (3, 64, 96)
        got = interpret(dev['img'], prm)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (seed, flags)
        seen |= flags
    assert seen == 2047                                  # every flag occurred


# ------------------------------------------------------------------------------------------------ 5. off = unchanged
def test_resize_behind_a_deferred_operation_still_raises():
    import transforms as T
    for mode in ('torch', 'exact'):
        d = T.RandomHorizontalFlip(prob=1.0, rng=np.random.default_rng(0))(T.DeferImage()(sample(random_frame(*SRC_HW, seed=1))))
        assert d['img_ops'] == [('flip', True)]
        with pytest.raises(NotImplementedError):
            T.Resize3D(TARGET_HW, interpolation=mode)(d)
    with pytest.raises(ValueError):
        T.Resize3D(TARGET_HW, interpolation='cubic')
    # the default keeps resampling on the host behind an empty DeferImage list
    d = T.Resize3D(TARGET_HW)(T.DeferImage()(sample(random_frame(*SRC_HW, seed=1))))
    assert d['img_ops'] == [] and d['img'].shape == TARGET_HW + (3,)


def test_default_lists_without_resize_are_todays_and_with_it_start_with_resize3d():
    import transforms as T
    from dataset.monocon_dataset import default_train_transforms, default_transforms
    aug = [T.PhotometricDistortion, T.RandomShift, T.RandomHorizontalFlip, T.RandomCrop3D]
    tail = [T.Normalize, T.Pad, T.ToTensor]
    kinds = lambda lst: [type(t) for t in lst]
    assert kinds(default_transforms()) == kinds(default_transforms(False, None)) == tail
    assert kinds(default_transforms(True)) == kinds(default_transforms(True, resize_hw=None)) == [T.DeferImage, T.DeferredImage]
    assert kinds(default_train_transforms()) == kinds(default_train_transforms(None, False, None)) == aug + tail
    assert kinds(default_train_transforms(None, True)) == kinds(default_train_transforms(None, True, resize_hw=None)) \
        == [T.DeferImage] + aug + [T.DeferredImage]
    assert default_train_transforms()[3].crop_size == (320, 960)

    assert kinds(default_transforms(False, (288, 960))) == [T.Resize3D] + tail
    assert kinds(default_transforms(True, (288, 960))) == [T.DeferImage, T.Resize3D, T.DeferredImage]
    assert kinds(default_train_transforms(None, False, (288, 960))) == [T.Resize3D] + aug + tail
    lst = default_train_transforms(None, True, (288, 960))
    assert kinds(lst) == [T.DeferImage, T.Resize3D] + aug + [T.DeferredImage]
    assert lst[1].target_hw == (288, 960) and lst[1].interpolation == 'exact'
    assert lst[5].crop_size == (288 * 320 // 375, 960 * 960 // 1242) == (245, 742)           # the reference's proportion


def test_datasets_take_resize_hw():
    """MonoConDataset(resize_hw=) on the kitti_mini tree: host and deferred samples of the validation and of the train split
    agree as in test 4, at the target's padded size; KITTIRawDataset takes the argument too"""
    from dataset.monocon_dataset import MonoConDataset
    for split in ("val", "train"):
        host = MonoConDataset(MINI, split, aug_rng=np.random.default_rng(4), resize_hw=(96, 320))[0]
        dev = MonoConDataset(MINI, split, aug_rng=np.random.default_rng(4), device_image=True, resize_hw=(96, 320))[0]
        assert tuple(host['img'].shape) == (3, 96, 320) and tuple(dev['img'].shape) == (384, 1248, 3)
        assert dev['img_metas']['pad_shape'] == host['img_metas']['pad_shape'] == (96, 320)
        metas_equal(host['img_metas'], dev['img_metas'])
        for k in host['label']:
            assert torch.equal(host['label'][k], dev['label'][k]), (split, k)
        assert int(dev['img_aug'][2]) & 1024
        assert torch.equal(interpret(dev['img'], dev['img_aug'].numpy()), host['img'])
    assert MonoConDataset(MINI, "val", device_image=True)[0]['img_metas'].get('scale_hw') is None


def test_config_key_defaults_to_off_and_merges_from_yaml(tmp_path):
    from config.monocon_configs import _C
    cfg = _C.clone()
    assert list(cfg.DATA.RESIZE_HW) == []
    path = tmp_path / "resized.yaml"
    path.write_text("DATA:\n  RESIZE_HW: [288, 960]\n")
    cfg.merge_from_file(str(path))
    assert list(cfg.DATA.RESIZE_HW) == [288, 960]
    assert list(_C.DATA.RESIZE_HW) == []


def test_infer_raw_cli_takes_target_hw():
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "monocon-pytorch_amd")
    r = subprocess.run([sys.executable, os.path.join(pkg, "infer_raw.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--target_hw", "--data_dir", "--calib_file", "--checkpoint_file", "--gpu_id", "--save_dir", "--fps", "--batch_size",
                 "--num_workers", "--test_thres"):
        assert flag in r.stdout, flag


def test_kitti_conversion_uses_each_images_own_scale():
    """convert_to_kitti_3d / convert_to_kitti_2d / img_hw_scale (the rows mc_kitti_format reads): image i is mapped back with
    ITS scale_hw -- a departure from the reference, which takes the batch's first: 375x1242 and 370x1224 frames resized to one
    target have different factors.  A batch that agrees gives what the first entry gave; a list of the wrong length raises."""
    from hipmonocon import synth
    from utils.kitti_convert_utils import convert_to_kitti_2d, convert_to_kitti_3d, img_hw_scale
    target = (288, 960)
    scales = [np.array(target) / np.array(hw) for hw in ((375, 1242), (370, 1224))]
    metas = {"ori_shape": [target, target], "sample_idx": [3, 4], "scale_hw": scales}
    box3d = torch.tensor([[1.0, 1.5, 20.0, 3.9, 1.5, 1.6, 0.3], [-3.0, 1.6, 12.0, 3.5, 1.4, 1.5, -1.2]])
    res3d = [{"boxes_3d": box3d, "scores_3d": torch.tensor([0.9, 0.8]), "labels_3d": torch.tensor([2, 0])}] * 2
    box2d = np.array([[100.0, 50.0, 300.0, 200.0, 0.9]], np.float32)
    res2d = [[box2d, np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32)]] * 2
    calibs = [synth.SynthCalib(), synth.SynthCalib()]
    plain = {k: v for k, v in metas.items() if k != "scale_hw"}
    k3, k3_plain = convert_to_kitti_3d(res3d, metas, calibs), convert_to_kitti_3d(res3d, plain, calibs)
    k2, k2_plain = convert_to_kitti_2d(res2d, metas), convert_to_kitti_2d(res2d, plain)
    rows = img_hw_scale(metas, 2)
    assert rows.dtype == np.float32 and rows.shape == (2, 4)
    for i, s in enumerate(scales):
        inv = np.array([1 / s[1], 1 / s[0]] * 2)
        assert len(k3[i]["name"]) == len(k3_plain[i]["name"]) > 0
        assert np.array_equal(k3[i]["bbox"], k3_plain[i]["bbox"] * inv)
        assert np.array_equal(k2[i]["bbox"], k2_plain[i]["bbox"] * inv)
        assert np.array_equal(rows[i], np.array([288, 960, inv[0], inv[1]], np.float32))
    assert not np.array_equal(k2[0]["bbox"], k2[1]["bbox"])                 # the two frames' factors do differ
    same = dict(metas, scale_hw=[scales[0], scales[0]])
    assert np.array_equal(convert_to_kitti_2d(res2d, same)[1]["bbox"], k2[0]["bbox"])
    assert np.array_equal(img_hw_scale(plain, 2)[:, 2:], np.ones((2, 2), np.float32))
    for fn in (lambda m: convert_to_kitti_3d(res3d, m, calibs), lambda m: convert_to_kitti_2d(res2d, m), lambda m: img_hw_scale(m, 2)):
        with pytest.raises(ValueError):
            fn(dict(metas, scale_hw=scales[:1]))


def test_deferred_resized_samples_must_share_a_canvas():
    """a deferred Resize3D keeps each frame on the canvas of its own size: frames that pad to different canvases cannot be
    stacked, and collate_fn says so (the host lists resize first and take such a batch)"""
    from dataset.monocon_dataset import MonoConDataset, default_transforms
    from transforms import Compose
    frames = [random_frame(75, 131, seed=1), random_frame(40, 131, seed=2)]

    def samples(device_image):
        lst = Compose(default_transforms(device_image, TARGET_HW))
        return [lst(sample(fr, i)) for i, fr in enumerate(frames)]

    assert tuple(MonoConDataset.collate_fn(samples(False))["img"].shape) == (2, 3, 64, 96)
    dev = samples(True)
    assert [tuple(d["img"].shape) for d in dev] == [(96, 160, 3), (64, 160, 3)]
    with pytest.raises(ValueError, match="canvases of different sizes"):
        MonoConDataset.collate_fn(dev)
