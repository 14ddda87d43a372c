"""Resize3D in the fused preprocess launch (`mc_preprocess_augmented`, flag 1024): the device output against the host pipeline
behind `Resize3D(interpolation='exact')`, every float32 bit.  The resample's arithmetic is pinned on the host in
tests/test_resize_host.py (`resize_bilinear_u8`); in the tests that launch the kernel on rows of their own the canvas OUTSIDE each
frame is filled with 255 instead of zeros, so that a tap that leaves the frame shows in the output.  The end-to-end tests at the
bottom (detect, the engine, infer_raw.py) take DeferredImage's samples as they come, i.e. zero-padded canvases: the 255 fill does
not apply there, tap clamping is the kernel-level tests' business."""
import numpy as np
import pytest
import torch

from test_resize_host import SRC_HW, TARGET_HW, host_and_deferred, random_frame, sample

pytestmark = pytest.mark.gpu


def _host_image(frame, target_hw):
    """Resize3D('exact') -> Normalize -> Pad -> ToTensor on the host: float32 (3, Hp, Wp)"""
    from dataset.monocon_dataset import IMG_MEAN, IMG_STD
    import transforms as T
    d = {"img": T.resize_bilinear_u8(frame, target_hw), "img_metas": {}}
    for t in (T.Normalize(mean=IMG_MEAN, std=IMG_STD), T.Pad(32), T.ToTensor()):
        d = t(d)
    return d["img"]


def _canvas(frame, canvas_hw):
    c = np.full(tuple(canvas_hw) + (3,), 255, np.uint8)
    c[:frame.shape[0], :frame.shape[1]] = frame
    return torch.from_numpy(c)


def _row(frame, target_hw):
    prm = np.zeros(24, np.float32)
    prm[0], prm[1], prm[2], prm[17], prm[18] = target_hw[0], target_hw[1], 1024, frame.shape[0], frame.shape[1]
    return torch.from_numpy(prm)


def _assert_bit_equal(got, want, what):
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    same = torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert same, (what, int((got != want).sum()), float((got - want).abs().max()))


def _resize_only(frames, canvas_hw, target_hw, pad_hw):
    from hipmonocon.engine import Engine
    f = torch.stack([_canvas(fr, canvas_hw) for fr in frames]).cuda()
    p = torch.stack([_row(fr, target_hw) for fr in frames]).cuda()
    got = Engine().preprocess_augmented(f, p, out_hw=pad_hw).cpu()
    assert tuple(got.shape) == (len(frames), 3) + tuple(pad_hw)
    for k, fr in enumerate(frames):
        _assert_bit_equal(got[k], _host_image(fr, target_hw), (k, fr.shape[:2], target_hw))


def test_resize_only_three_source_sizes_in_one_launch():
    """37x61, 35x59 and 33x64 in one 64x64 canvas -> 45x83, padded to 64x96: an inexact ratio, every frame with its own size,
    the last rows / columns clamp their second tap to the frame's edge"""
    frames = [random_frame(h, w, seed=20 + i) for i, (h, w) in enumerate(((37, 61), (35, 59), (33, 64)))]
    _resize_only(frames, (64, 64), (45, 83), (64, 96))


@pytest.mark.parametrize("src_hw,target_hw,pad_hw", [((75, 131), (31, 50), (32, 64)), ((40, 131), (64, 50), (64, 64))])
def test_scale_directions(src_hw, target_hw, pad_hw):
    """down in both axes; up in y and down in x"""
    canvas = (-(-src_hw[0] // 32) * 32, -(-src_hw[1] // 32) * 32)
    _resize_only([random_frame(*src_hw, seed=30), random_frame(*src_hw, seed=31)], canvas, target_hw, pad_hw)


def test_all_stages_equal_the_host_pipeline():
    """resize + colour + shift + flip + window, the lists of tests/test_resize_host.py (test 4) over 12 seeds in one launch: the
    device output is the host pipeline's image"""
    from hipmonocon.engine import Engine
    frames, params, want, seen = [], [], [], 0
    for seed in range(12):
        host, dev, frame = host_and_deferred(seed)
        assert tuple(dev["img"].shape) == (96, 160, 3) and dev["img_metas"]["pad_shape"] == (64, 96)
        frames.append(_canvas(frame, (96, 160))); params.append(dev["img_aug"]); want.append(host["img"])
        seen |= int(dev["img_aug"][2])
    assert seen == 2047
    got = Engine().preprocess_augmented(torch.stack(frames).cuda(), torch.stack(params).cuda(), out_hw=(64, 96)).cpu()
    for k in range(len(want)):
        _assert_bit_equal(got[k], want[k], (k, int(params[k][2])))


def test_full_size_once():
    """370x1224 -> 384x1280, B=2: the size at which a contracted multiply-add in the resample shows (a few of 1.47 M values)"""
    _resize_only([random_frame(370, 1224, seed=40), random_frame(370, 1224, seed=41)], (384, 1248), (384, 1280), (384, 1280))


def test_without_the_bit_a_row_means_what_it_meant():
    """out_hw=None and rows without the resize bit: the output has the canvas's size and is mc_preprocess of the frames"""
    from hipmonocon.engine import Engine
    from dataset.monocon_dataset import IMG_MEAN, IMG_STD
    import transforms as T
    frames = [random_frame(37, 61, seed=60), random_frame(64, 64, seed=61)]
    rows = []
    for fr in frames:
        prm = np.zeros(24, np.float32)
        prm[0], prm[1] = fr.shape[:2]
        rows.append(torch.from_numpy(prm))
    got = Engine().preprocess_augmented(torch.stack([_canvas(fr, (64, 64)) for fr in frames]).cuda(), torch.stack(rows).cuda(), out_hw=None).cpu()
    assert tuple(got.shape) == (2, 3, 64, 64)
    for k, fr in enumerate(frames):
        d = {"img": fr, "img_metas": {}}
        for t in (T.Normalize(mean=IMG_MEAN, std=IMG_STD), T.Pad(32), T.ToTensor()):
            d = t(d)
        want = torch.zeros(3, 64, 64)
        want[:, :d["img"].shape[1], :d["img"].shape[2]] = d["img"]
        _assert_bit_equal(got[k], want, k)


def test_detect_on_a_deferred_resized_batch(golden_sd):
    """two 75x131 frames resized to 64x96: MonoConDetector.detect on the collated deferred batch (finish_batch takes the output
    size from pad_shape) gives the KITTI rows of the same frames resized on the host and fed as float32; the rows are in the
    source frame's coordinates (scale_hw applied: the boxes of a run without it, times the inverse factors).  The canvases are
    DeferredImage's own, zero-padded: no 255 fill here."""
    from dataset.monocon_dataset import MonoConDataset, default_transforms
    from model import MonoConDetector
    from model.detector.monocon_detector import default_test_config
    from transforms import Compose
    m = MonoConDetector(34, pretrained_backbone=False, test_config=dict(default_test_config, test_thres=0.0))
    m.load_state_dict(golden_sd, strict=True)
    m = m.cuda().eval()
    frames = [random_frame(*SRC_HW, seed=70), random_frame(*SRC_HW, seed=71)]

    def batch(device_image):
        lst = Compose(default_transforms(device_image, TARGET_HW))
        samples = []
        for i, fr in enumerate(frames):
            d = sample(fr, i)
            del d["label"]
            samples.append(lst(d))
        b = MonoConDataset.collate_fn(samples)
        b["img"] = b["img"].cuda()
        if device_image:
            b["img_aug"] = b["img_aug"].cuda()
        return b

    host, dev = batch(False), batch(True)
    assert dev["img"].dtype == torch.uint8 and tuple(dev["img"].shape) == (2, 96, 160, 3)
    assert host["img"].dtype == torch.float32 and tuple(host["img"].shape) == (2, 3, 64, 96)
    unscaled = dict(host, img_metas={k: v for k, v in host["img_metas"].items() if k != "scale_hw"})
    with torch.no_grad():
        want = m.detect(dict(host))
        got = m.detect(dev)
        plain = m.detect(unscaled)
    assert dev["img"].dtype == torch.float32 and torch.equal(dev["img"], host["img"]) and "img_aug" not in dev
    inv = np.array([SRC_HW[1] / TARGET_HW[1], SRC_HW[0] / TARGET_HW[0]] * 2)
    for field in ("img_bbox", "img_bbox2d"):
        assert sum(len(a["name"]) for a in want[field]) > 0
        for a, b, c in zip(got[field], want[field], plain[field]):
            assert a.keys() == b.keys()
            for k in a:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (field, k)
            assert list(a["name"]) == list(c["name"])
            assert np.allclose(a["bbox"], c["bbox"] * inv, rtol=1e-6, atol=1e-6)

    uneven = dict(batch(True))
    uneven["img_metas"] = dict(uneven["img_metas"], pad_shape=[(64, 96), (96, 160)])
    from hipmonocon.lib import MonoconHipError
    with pytest.raises(MonoconHipError):
        m.finish_batch(uneven)


def test_engine_runs_at_the_configured_resolution(tmp_path):
    """config DATA.RESIZE_HW on the kitti_mini tree, one loader worker: deferred frames of the decoded size through RingLoader
    and DevicePrefetcher (the labels are checked against pad_shape, not the canvas), the train step and the evaluation at
    192x640"""
    import os
    from engine.monocon_engine import MonoconEngine
    from hipmonocon.feed import RingLoader
    from test_engine import small_cfg
    cfg = small_cfg(tmp_path, epochs=1)
    cfg.DATA.ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_mini")
    cfg.DATA.BATCH_SIZE = 2
    cfg.DATA.NUM_WORKERS = 1
    cfg.DATA.RESIZE_HW = [192, 640]
    eng = MonoconEngine(cfg)
    assert isinstance(eng.train_loader, RingLoader)
    assert (eng.train_loader.ring.dtype, tuple(eng.train_loader.ring.shape[1:])) == (torch.uint8, (2, 384, 1248, 3))
    batch = next(iter(eng.test_loader))
    assert batch["img_metas"]["pad_shape"] == [(192, 640)] * 2 and batch["img_metas"]["ori_shape"] == [(192, 640)] * 2
    assert tuple(eng.model.finish_batch({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()})["img"].shape) == (2, 3, 192, 640)
    eng.train()
    assert len(eng.entire_losses) == 1 and eng.entire_losses[0] == eng.entire_losses[0]
    ap = eng.evaluate()
    assert len(ap) == 4 * 21 and all(0.0 <= v <= 100.0 for v in ap.values())


def test_infer_raw_at_a_target_resolution(golden_sd, tmp_path):
    """`infer_raw.py --target_hw 192 640` over a 3-frame raw drive (batch 2, one loader worker, threshold 0): the label files
    are those of the same frames resized on the host with 'exact', one at a time, through detect -- names and order exact,
    values within the tolerance tests/test_hip_kitti_format.py grants two batch sizes of one forward (rtol 1e-5, atol 2e-4) --
    and their boxes are the resized frame's times each frame's OWN inverse resize factors (source-frame coordinates)"""
    import os
    import subprocess
    import sys
    from conftest import PKG
    from dataset.kitti_raw_dataset import KITTIRawDataset
    from model import MonoConDetector
    from model.detector.monocon_detector import default_test_config
    from test_kitti_raw import make_raw_drive
    from utils.kitti_convert_utils import kitti_result_lines
    img_dir, calib = make_raw_drive(tmp_path / "drive", 3)
    ckpt, out = str(tmp_path / "seed7.pth"), str(tmp_path / "out")
    torch.save({"state_dict": {"model": golden_sd}}, ckpt)
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(PKG, "infer_raw.py"), "--data_dir", img_dir,
           "--calib_file", calib, "--checkpoint_file", ckpt, "--save_dir", out, "--batch_size", "2", "--num_workers", "1",
           "--test_thres", "0.0", "--target_hw", "192", "640"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])

    def parse(lines):
        rows = [ln.split() for ln in lines if ln.strip()]
        return [row[0] for row in rows], np.array([[float(v) for v in row[1:]] for row in rows]).reshape(len(rows), 15)

    m = MonoConDetector(34, pretrained_backbone=False, test_config=dict(default_test_config, test_thres=0.0))
    m.load_state_dict(golden_sd, strict=True)
    m = m.cuda().eval()
    ds = KITTIRawDataset(img_dir, calib, resize_hw=(192, 640))
    P2 = ds.calib.P2.copy()
    scales = set()
    for i, path in enumerate(ds.image_files):
        src_h, src_w = ds.load_image(i).shape[:2]
        with open(os.path.join(out, os.path.splitext(os.path.basename(path))[0] + ".txt")) as f:
            names, vals = parse(f.readlines())
        d = ds[i]
        assert tuple(d["img"].shape) == (1, 3, 192, 640) and d["img_metas"]["ori_shape"] == [(192, 640)]
        d["img"] = d["img"].cuda()
        unscaled = dict(d, img_metas={k: v for k, v in d["img_metas"].items() if k != "scale_hw"})
        with torch.no_grad():
            ref_names, ref_vals = parse(kitti_result_lines(m.detect(d)["img_bbox"][0]))
            plain = m.detect(unscaled)["img_bbox"][0]
        assert len(names) > 0 and names == ref_names == list(plain["name"]), path
        assert np.allclose(vals, ref_vals, rtol=1e-5, atol=2e-4), (path, float(np.abs(vals - ref_vals).max()))
        # the boxes of the resized frame times THIS frame's inverse factors (the drive's frames have two sizes, the batch is 2);
        # 3e-4: the files' four decimals (5e-5) and two float32 roundings of a coordinate below 1300 (2 x 8e-5); + what the
        # line above grants a forward at another batch size (rtol 1e-5, atol 2e-4), through a factor of at most 2
        inv = np.array([src_w / 640, src_h / 192] * 2)
        assert np.allclose(vals[:, 3:7], plain["bbox"] * inv, rtol=1e-5, atol=7e-4), (path, float(np.abs(vals[:, 3:7] - plain["bbox"] * inv).max()))
        scales.add((src_h, src_w))
    assert len(scales) == 2
    assert np.array_equal(ds.calib.P2, P2)               # each sample rescaled its own copy of the drive's calibration
