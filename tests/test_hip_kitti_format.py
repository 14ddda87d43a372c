"""mc_kitti_format (the KITTI result rows of a decoded batch on the device), MonoConDetector.detect and test_raw.py end to end.
GPU-only; the host side of the raw-drive path is tests/test_kitti_raw.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, load_golden
from test_kitti_raw import make_raw_drive

pytestmark = pytest.mark.gpu

FIELDS = ("alpha", "bbox", "dimensions", "location", "rotation_y", "score", "sample_idx")


@pytest.fixture(scope="module")
def eng():
    from hipmonocon.engine import Engine
    return Engine()


def run_format(eng, box2d, box3d, cls, keep, P2, hws, sample_idx):
    """upload, one mc_kitti_format launch, the detector's row builder"""
    from utils.kitti_convert_utils import kitti_annos_from_rows
    dev = eng.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    R = {"box2d": up(box2d), "box3d": up(box3d), "cls": up(cls.astype(np.int64)), "keep_thr": up(keep.astype(np.uint8))}
    F = eng.kitti_format(R, up(P2.astype(np.float32)), up(hws.astype(np.float32)))
    h = {k: v.cpu().numpy() for k, v in F.items() if k != "packed"}
    return kitti_annos_from_rows(h["rows3d"], h["n3d"], h["rows2d"], h["n2d"], sample_idx), h


def assert_annos_close(got, ref, tag=""):
    assert len(got) == len(ref)
    for i, (a, r) in enumerate(zip(got, ref)):
        assert list(a["name"]) == list(r["name"]), (tag, i)
        for k in FIELDS:
            x, y = np.asarray(a[k], np.float64), np.asarray(r[k], np.float64)
            assert x.shape == y.shape, (tag, i, k, x.shape, y.shape)
            assert np.allclose(x, y, rtol=1e-5, atol=1e-4), (tag, i, k, float(np.abs(x - y).max()) if x.size else 0.0)


def test_kitti_format_vs_reference_golden(eng):
    """the reference decode of tests/golden/decode_k30.npz, laid out as mc_decode leaves it (kept rows between discarded
    ones), against the reference's own KITTI annotation dicts"""
    from hipmonocon import synth
    from utils.kitti_convert_utils import CLASSES
    g = load_golden("decode_k30.npz")
    B, K = 4, 64
    rng = np.random.default_rng(0)
    box2d = rng.uniform(-50, 1300, (B, K, 5)).astype(np.float32)           # discarded rows: garbage
    box3d = rng.uniform(-20, 20, (B, K, 7)).astype(np.float32)
    cls = rng.integers(0, 3, (B, K))
    keep = np.zeros((B, K), bool)
    for i in range(B):
        b2, b3, lab = g["box2d.%d" % i], g["box3d.%d" % i], g["label.%d" % i]
        slots = np.sort(rng.choice(K, len(b2), replace=False))
        box2d[i, slots], box3d[i, slots], cls[i, slots], keep[i, slots] = b2, b3, lab, True
    P2 = np.stack([synth.SynthCalib().P2] * B)
    hws = np.tile(np.array([375, 1242, 1, 1], np.float32), (B, 1))
    got, _ = run_format(eng, box2d, box3d, cls, keep, P2, hws, [11, 12, 13, 14])
    for field in ("img_bbox", "img_bbox2d"):
        for i in range(B):
            a = got[field][i]
            assert [CLASSES.index(n) for n in a["name"]] == g["kitti.%s.%d.name" % (field, i)].tolist(), (field, i)
            for k in FIELDS:
                ref = g["kitti.%s.%d.%s" % (field, i, k)]
                x = np.asarray(a[k], np.float64)
                assert x.shape == ref.shape, (field, i, k)
                assert np.allclose(x, ref, rtol=1e-5, atol=1e-4), (field, i, k)


def _corner_depths(boxes, P2):
    """projected depth of the 8 corners, as project_boxes_3d forms them"""
    unit = np.array([[sx, sy, sz] for sx in (-0.5, 0.5) for sy in (-1.0, 0.0) for sz in (-0.5, 0.5)], np.float32)
    c = boxes[:, None, 3:6] * unit[None]
    s, co = np.sin(boxes[:, 6])[:, None], np.cos(boxes[:, 6])[:, None]
    pts = np.stack([c[..., 0] * co + c[..., 2] * s, c[..., 1], -c[..., 0] * s + c[..., 2] * co], -1) + boxes[:, None, :3]
    P = np.asarray(P2, np.float64)
    return pts.astype(np.float64) @ P[2, :3] + P[2, 3]


@pytest.mark.parametrize("K", [100, 1024])
def test_kitti_format_vs_host_conversion_on_real_decode(eng, K):
    """mc_decode at B=64, then mc_kitti_format against convert_to_kitti_3d / _2d on the same decode output: per-image P2,
    mixed original shapes, a resize factor, images without a kept box, boxes outside the image, clipped and behind the
    camera.  Counts and row order exact, floats to rtol 1e-5 / atol 1e-4."""
    from hipmonocon import synth
    from hipmonocon.engine import p2_inverse
    from utils.kitti_convert_utils import convert_to_kitti_2d, convert_to_kitti_3d, img_hw_scale, project_boxes_3d
    B, H, W = 64, 96, 312
    rng = np.random.default_rng(K)
    d = synth.make_decode_inputs(40 + K, B, H, W, topk=K)
    P2 = np.stack([synth.KITTI_P2] * B).astype(np.float64)
    P2[:, 0, 0] *= rng.uniform(0.97, 1.03, B)
    P2[:, 1, 1] = P2[:, 0, 0]
    P2[:, 0, 2] += rng.uniform(-15, 15, B)
    P2[:, 1, 2] += rng.uniform(-8, 8, B)
    P2 = P2.astype(np.float32)
    dev = eng.device
    pred = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    R = eng.decode(pred, torch.from_numpy(P2).to(dev), torch.from_numpy(p2_inverse(P2)).to(dev), (4 * H, 4 * W), K, 0.25)
    box2d, box3d = R["box2d"].cpu().numpy(), R["box3d"].cpu().numpy()
    cls, keep = R["cls"].cpu().numpy(), R["keep_thr"].cpu().numpy().astype(bool)
    keep[[3, 17, 40]] = False                                             # images without a kept box
    # injected geometry on kept rows: boxes straddling the camera plane, boxes far to the side (outside every frame)
    for i in range(B):
        rows = np.flatnonzero(keep[i])
        if len(rows) >= 8:
            bh = rows[:3]
            box3d[i, bh, 2] = rng.uniform(0.3, 1.2, len(bh))
            box3d[i, bh, 3] = rng.uniform(3.0, 5.0, len(bh))
            fo = rows[3:5]
            box3d[i, fo, 0] = rng.choice([-1.0, 1.0], len(fo)) * rng.uniform(80, 120, len(fo))
            box3d[i, fo, 2] = rng.uniform(8, 20, len(fo))
    ori = np.stack([rng.integers(300, 4 * H + 1, B), rng.integers(1000, 4 * W + 1, B)], 1)
    metas = {"ori_shape": [tuple(int(v) for v in o) for o in ori], "sample_idx": list(range(100, 100 + B)),
             "scale_hw": [(0.8, 0.9)] * B}
    # margin: every quantity the visibility test reads is >= 1e-3 px from its bound and no corner lies within 1e-2 of the
    # camera plane, so that a last-bit difference of sinf / atan2f cannot flip a row; the few kept rows that miss it are
    # dropped from the input of both paths
    n_near = 0
    for i in range(B):
        rows = np.flatnonzero(keep[i])
        if not len(rows):
            continue
        b2 = project_boxes_3d(box3d[i, rows], P2[i])
        h, w = ori[i]
        gap = np.min(np.abs(np.stack([b2[:, 0] - w, b2[:, 1] - h, b2[:, 2], b2[:, 3]], 1)), 1)
        zc = np.abs(_corner_depths(box3d[i, rows], P2[i])).min(1)
        bad = ~((gap >= 1e-3) & (zc >= 1e-2))
        n_near += int(bad.sum())
        keep[i, rows[bad]] = False
    assert n_near <= max(8, keep.sum() // 50), n_near
    # the categories are there
    cats = dict(outside=0, clipped=0, inside=0, behind=0)
    for i in range(B):
        rows = np.flatnonzero(keep[i])
        if not len(rows):
            continue
        b2 = project_boxes_3d(box3d[i, rows], P2[i])
        h, w = ori[i]
        vis = (b2[:, 0] < w) & (b2[:, 1] < h) & (b2[:, 2] > 0) & (b2[:, 3] > 0)
        inside = (b2[:, 0] >= 0) & (b2[:, 1] >= 0) & (b2[:, 2] <= w) & (b2[:, 3] <= h)
        cats["outside"] += int((~vis).sum())
        cats["inside"] += int((vis & inside).sum())
        cats["clipped"] += int((vis & ~inside).sum())
        cats["behind"] += int((_corner_depths(box3d[i, rows], P2[i]) < 0).any(1).sum())
    assert all(v > 0 for v in cats.values()), cats
    assert not keep[3].any() and keep.sum() > B

    res3d = [{"boxes_3d": torch.from_numpy(box3d[i][keep[i]]), "scores_3d": torch.from_numpy(box2d[i][keep[i]][:, 4]),
              "labels_3d": torch.from_numpy(cls[i][keep[i]])} for i in range(B)]
    res2d = [[box2d[i][keep[i] & (cls[i] == c)] for c in range(3)] for i in range(B)]
    ref3 = convert_to_kitti_3d(res3d, metas, [synth.SynthCalib(P2[i]) for i in range(B)])
    ref2 = convert_to_kitti_2d(res2d, metas)
    got, h = run_format(eng, box2d, box3d, cls, keep, P2, img_hw_scale(metas, B), metas["sample_idx"])
    assert h["n3d"].tolist() == [len(r["name"]) for r in ref3]
    assert h["n2d"].tolist() == [len(r["name"]) for r in ref2]
    assert_annos_close(got["img_bbox"], ref3, "3d")
    assert_annos_close(got["img_bbox2d"], ref2, "2d")


def test_kitti_format_rejects_bad_arguments(eng):
    from hipmonocon import lib
    dev = eng.device
    R = {"box2d": torch.zeros(2, 8, 5, device=dev), "box3d": torch.zeros(2, 8, 7, device=dev),
         "cls": torch.zeros(2, 8, dtype=torch.int64, device=dev), "keep_thr": torch.zeros(2, 8, dtype=torch.uint8, device=dev)}
    P2, hws = torch.zeros(2, 3, 4, device=dev), torch.zeros(2, 4, device=dev)
    with pytest.raises(lib.MonoconHipError):
        eng.kitti_format(R, P2[:1], hws)                                   # shape mismatch, caught before the launch
    with pytest.raises(lib.MonoconHipError):
        eng.kitti_format(dict(R, cls=R["cls"].int()), P2, hws)
    import ctypes as C
    nul = C.c_void_p(0)
    p = lambda t: C.c_void_p(t.data_ptr())
    out = torch.empty(2 * 1025 * 20 + 4, device=dev)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for B, K in ((0, 8), (2, 0), (2, 1025)):
        rc = eng.lib.mc_kitti_format(eng.h, p(R["box2d"]), p(R["box3d"]), p(R["cls"]), p(R["keep_thr"]), p(P2), p(hws), B, K,
                                     p(out), p(out), p(out), p(out), s)
        assert rc != 0 and b"bad shape" in eng.lib.mc_last_error(eng.h)
    rc = eng.lib.mc_kitti_format(eng.h, nul, p(R["box3d"]), p(R["cls"]), p(R["keep_thr"]), p(P2), p(hws), 2, 8,
                                 p(out), p(out), p(out), p(out), s)
    assert rc != 0 and b"null" in eng.lib.mc_last_error(eng.h)


def _detector(sd, thres):
    from model import MonoConDetector
    from model.detector.monocon_detector import default_test_config
    m = MonoConDetector(34, pretrained_backbone=False, test_config=dict(default_test_config, test_thres=thres))
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _assert_vis_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in ("boxes_3d", "scores_3d", "labels_3d"):
            assert x["img_bbox"][k].dtype == y["img_bbox"][k].dtype and torch.equal(x["img_bbox"][k], y["img_bbox"][k]), k
        assert len(x["img_bbox2d"]) == len(y["img_bbox2d"]) == 3
        for p, q in zip(x["img_bbox2d"], y["img_bbox2d"]):
            assert p.dtype == q.dtype and np.array_equal(p, q)


@pytest.mark.parametrize("thres", [0.0, 0.4])
def test_detect_matches_batch_eval(golden_sd, thres):
    """seed-7 synthetic weights: detect's visualiser list is batch_eval's bit for bit, its KITTI dicts the host
    conversion's to rtol 1e-5 / atol 1e-4 (names, counts and order exact)"""
    from hipmonocon import synth
    m = _detector(golden_sd, thres)
    batch = synth.make_batch(77, 4, 96, 320, with_labels=False)
    batch["img_metas"]["ori_shape"] = [(90, 310), (96, 320), (80, 300), (96, 256)]
    batch["img_metas"]["sample_idx"] = [5, 6, 7, 8]
    batch["img"] = batch["img"].cuda()
    with torch.no_grad():
        vis_ref = m.batch_eval(dict(batch), get_vis_format=True)
        kitti_ref = m.batch_eval(dict(batch))
        vis = m.detect(dict(batch), get_vis_format=True)
        kitti = m.detect(dict(batch))
        kitti2, vis2 = m.detect_with_vis(dict(batch))
    assert sum(len(v["img_bbox"]["boxes_3d"]) for v in vis_ref) > 0
    _assert_vis_equal(vis, vis_ref)
    _assert_vis_equal(vis2, vis_ref)
    for got in (kitti, kitti2):
        assert set(got) == {"img_bbox", "img_bbox2d"}
        assert_annos_close(got["img_bbox"], kitti_ref["img_bbox"], "3d")
        assert_annos_close(got["img_bbox2d"], kitti_ref["img_bbox2d"], "2d")


def _parse_label_file(path):
    with open(path) as f:
        rows = [ln.split() for ln in f if ln.strip()]
    return [r[0] for r in rows], np.array([[float(v) for v in r[1:]] for r in rows]).reshape(len(rows), 15)


def test_test_raw_end_to_end(golden_sd, tmp_path):
    """test_raw.py over a 5-frame raw drive (batch 2: the last batch is partial, one loader worker, threshold 0) against
    the same frames through KITTIRawDataset's batch-of-one samples, batch_eval and the host conversion"""
    from dataset.kitti_raw_dataset import KITTIRawDataset
    from utils.kitti_convert_utils import kitti_result_lines
    img_dir, calib = make_raw_drive(tmp_path / "drive", 5)
    ckpt = str(tmp_path / "seed7.pth")
    torch.save({"state_dict": {"model": golden_sd}}, ckpt)
    out = str(tmp_path / "out")
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(PKG, "test_raw.py"), "--data_dir", img_dir,
           "--calib_file", calib, "--checkpoint_file", ckpt, "--save_dir", out, "--batch_size", "2", "--num_workers", "1",
           "--test_thres", "0.0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "--fps" in r.stdout
    ds = KITTIRawDataset(img_dir, calib)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in ds.image_files]
    assert sorted(f for f in os.listdir(out) if f.endswith(".txt")) == [s + ".txt" for s in stems]
    vis = torch.load(os.path.join(out, "vis_results.pt"), weights_only=False)
    assert len(vis) == 5
    m = _detector(golden_sd, 0.0)
    for i, stem in enumerate(stems):
        names, vals = _parse_label_file(os.path.join(out, stem + ".txt"))
        assert len(names) > 0, stem
        d = ds[i]
        d["img"] = d["img"].cuda()
        d["img_metas"]["ori_shape"] = [d["img_metas"]["ori_shape"][0][:2]]
        d["img_metas"]["sample_idx"] = [i]
        with torch.no_grad():
            ref = m.batch_eval(d)["img_bbox"][0]
        ref_names, ref_vals = _parse_label_file_lines(kitti_result_lines(ref))
        assert names == ref_names, stem
        assert np.allclose(vals, ref_vals, rtol=1e-5, atol=2e-4), (stem, float(np.abs(vals - ref_vals).max()))
        assert len(vis[i]["img_bbox"]["boxes_3d"]) >= len(names)


def _parse_label_file_lines(lines):
    rows = [ln.split() for ln in lines]
    return [r[0] for r in rows], np.array([[float(v) for v in r[1:]] for r in rows]).reshape(len(rows), 15)
