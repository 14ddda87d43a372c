"""SURVEY 8f-4 pinned to the reference's own source (round 6; tests/golden/make_f4_golden.py, meta_f4.json).

The goldens were produced by the REFERENCE'S code imported under inert placeholders for cv2 / numba (identity decorators,
no placeholder function ever ran -- the generator asserts an empty access log): Normalize / Pad / ToTensor, the label loop
and collate of MonoConDataset, and the host side of the KITTI AP evaluator (ignore rules, matching, recall thresholds,
eval_class, AP40, the result dict and table).  For the BEV / 3D metrics of these goldens the reference's evaluator ran on
rotated overlaps supplied by the oracle; the reference's float32 numba.cuda rotated-overlap kernel itself is pinned
separately (make_rotate_iou_golden.py, tests/test_rotate_iou_reference.py).

Held to these goldens here: the oracle's restatements (CPU) and the product's host code (CPU: transforms, dataset,
native matching library); the device paths (mc_preprocess, HIP overlaps inside kitti_eval) under ``-m gpu``."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from hipmonocon import synth
from oracle import kitti_eval_oracle as KO
from oracle import monocon_oracle as O

SIZES = [(375, 1242), (370, 1224), (384, 1280), (33, 65), (64, 96)]
MINI = os.path.join(GOLDEN, "kitti_mini")


def _frame(i, h, w, dt):
    a = synth.uniform(31 + i, "raw", (h, w, 3), 0.0, 255.0).astype(np.float32)
    return np.floor(a).astype(np.uint8) if dt == "uint8" else a


def _check_img(g, tag, t):
    assert list(t.shape) == g[tag + "shape"].tolist() and str(t.dtype) == str(g[tag + "dtype"])
    if tag + "full" in g.files:
        assert np.array_equal(t.numpy(), g[tag + "full"])
    else:
        assert np.array_equal(t.reshape(-1)[::997].numpy(), g[tag + "samples"])
    assert zlib.crc32(t.contiguous().numpy().tobytes()) == int(g[tag + "crc32"])        # the whole tensor, bit for bit


def test_generator_ran_the_reference_without_touching_a_placeholder():
    meta = json.load(open(os.path.join(GOLDEN, "meta_f4.json")))
    assert meta["placeholder_attribute_accesses"] == []
    assert all(p.startswith("/root/reference/") for p in meta["reference_modules_run"])
    # every reference function the evaluator calls has run somewhere: the rotated IoU in its own generator
    assert meta["not_executed"] == [] and "rotate_iou_ref.npz" in meta["rotated_iou"]
    rmeta = json.load(open(os.path.join(GOLDEN, "meta_rotate_iou.json")))
    assert "rotate_iou_kernel_eval (emulated launch, float32)" in rmeta["executed"]
    assert all(p.startswith("/root/reference/") and p.endswith(("rotate_iou.py", "eval.py")) for p in rmeta["reference_modules_run"])
    assert os.path.getsize(os.path.join(GOLDEN, "rotate_iou_ref.npz")) > 0


def test_oracle_preprocess_is_the_reference_transform_chain():
    """oracle.preprocess == reference Normalize -> Pad -> ToTensor, bit for bit (uint8 and float32 frames, five sizes)"""
    g = load_golden("f4_transforms.npz")
    for i, (h, w) in enumerate(SIZES):
        for dt in ("uint8", "float32"):
            t, pad = O.preprocess(_frame(i, h, w, dt))
            tag = "%dx%d.%s." % (h, w, dt)
            assert list(pad) == g[tag + "pad_shape"].tolist()
            _check_img(g, tag, t)


def test_product_transforms_are_the_reference_transform_chain():
    """the product's transforms.Normalize / Pad / ToTensor (incl. ToTensor's label branch) vs the same golden"""
    import transforms as T
    g = load_golden("f4_transforms.npz")
    tf = T.Compose([T.Normalize(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375]), T.Pad(size_divisor=32), T.ToTensor()])
    for i, (h, w) in enumerate(SIZES):
        for dt in ("uint8", "float32"):
            d = tf({"img": _frame(i, h, w, dt), "img_metas": {"ori_shape": (h, w)},
                    "label": {"gt_bboxes": np.arange(8, dtype=np.float32).reshape(2, 4), "mask": np.array([True, False])}})
            tag = "%dx%d.%s." % (h, w, dt)
            assert list(d["img_metas"]["pad_shape"]) == g[tag + "pad_shape"].tolist()
            _check_img(g, tag, d["img"])
            if i == 3 and dt == "uint8":
                assert np.array_equal(d["label"]["gt_bboxes"].numpy(), g["label.gt_bboxes"])
                assert np.array_equal(d["label"]["mask"].numpy(), g["label.mask"])
                assert str(d["label"]["mask"].dtype) == str(g["label.mask.dtype"])


def test_product_dataset_label_loop_matches_the_reference_dataset():
    """MonoConDataset.__getitem__ on the mini tree vs the reference's own __getitem__ (filters, label assembly, key-point
    visibility flags, transforms) and collate_fn.  Integer-valued labels, masks, 2D boxes and the image are exact; the
    camera-frame quantities agree to float32 round-off (the product views an object in a frame, the reference converts
    its stored state back and forth in float32 -- see test_calibration_and_objects_match_the_reference_classes)."""
    from dataset.monocon_dataset import MonoConDataset
    g = load_golden("f4_dataset.npz")
    ds = MonoConDataset(MINI, "val")
    assert ds.file_prefix == g["ids"].tolist()
    samples = []
    for i, pid in enumerate(ds.file_prefix):
        s = ds[i]
        samples.append(s)
        assert list(s["img"].shape) == g[pid + ".img.shape"].tolist()
        assert np.array_equal(s["img"].reshape(-1)[::997].numpy(), g[pid + ".img.samples"])
        assert zlib.crc32(s["img"].contiguous().numpy().tobytes()) == int(g[pid + ".img.crc32"])
        assert list(s["img_metas"]["pad_shape"]) == g[pid + ".pad_shape"].tolist()
        assert list(s["img_metas"]["ori_shape"]) == g[pid + ".ori_shape"].tolist()
        assert s["img_metas"]["sample_idx"] == int(g[pid + ".sample_idx"])
        lab = s["label"]
        keys = sorted(k[len(pid) + 7:] for k in g.files if k.startswith(pid + ".label.") and not k.endswith(".dtype"))
        assert sorted(lab.keys()) == keys
        for k in keys:
            want = g["%s.label.%s" % (pid, k)]
            got = lab[k].numpy()
            assert got.shape == want.shape and str(lab[k].dtype) == str(g["%s.label.%s.dtype" % (pid, k)]), k
            if k in ("gt_bboxes", "gt_labels", "gt_labels_3d", "gt_kpts_valid_mask", "mask"):
                assert np.array_equal(got, want), (pid, k)
            elif k in ("centers2d", "gt_kpts_2d"):
                assert np.allclose(got, want, rtol=1e-5, atol=2e-3), (pid, k)          # pixels
            else:
                assert np.allclose(got, want, rtol=2e-6, atol=2e-6), (pid, k)
    b = MonoConDataset.collate_fn([samples[0], samples[0]])
    assert list(b["img"].shape) == g["collate.img.shape"].tolist()
    assert sorted(b.keys()) == g["collate.keys"].tolist() and sorted(b["img_metas"].keys()) == g["collate.meta_keys"].tolist()
    for k, v in b["label"].items():
        assert list(v.shape) == g["collate.label.%s.shape" % k].tolist()


# ------------------------------------------------------------------------------------------------ AP evaluator
def _per_frame_cases(g):
    gts, dts = synth.random_kitti_annos(11, frames=14)
    for cls in range(3):
        for diff in range(3):
            for f, (gt, dt) in enumerate(zip(gts, dts)):
                yield "f%d.c%d.d%d." % (f, cls, diff), cls, diff, gt, dt


def _frame_data(gt, dt):
    gd = np.concatenate([gt["bbox"], gt["alpha"][:, None]], 1).reshape(-1, 5)
    dd = np.concatenate([dt["bbox"].reshape(-1, 4), dt["alpha"].reshape(-1, 1), dt["score"].reshape(-1, 1)], 1)
    return gd, dd


@pytest.mark.parametrize("impl", ["oracle", "product"])
def test_ignore_rules_matching_and_thresholds_match_the_reference(impl):
    """per frame, for every (class, difficulty): clean_data, compute_statistics_jit in both passes (incl. DontCare
    absorption and orientation similarity), plus image_box_overlap for the four criteria, get_thresholds, get_split_parts
    -- against what the reference's own functions returned"""
    g = load_golden("f4_kitti_eval.npz")
    if impl == "product":
        from engine.kitti_eval import eval as E
    gts, dts = synth.random_kitti_annos(11, frames=14)
    for crit in (-1, 0, 1, 2):
        ov = (KO.image_overlap if impl == "oracle" else E.image_box_overlap)(gts[0]["bbox"], dts[0]["bbox"], crit)
        assert np.array_equal(ov, g["image_overlap.c%d" % crit])
    n = 0
    for tag, cls, diff, gt, dt in _per_frame_cases(g):
        gd, dd = _frame_data(gt, dt)
        if impl == "oracle":
            nv, ig, idt, dc = KO.clean(gt, dt, cls, diff)
        else:
            nv, ig, idt, dc = E.clean_data(gt, dt, cls, diff)
        assert nv == int(g[tag + "num_valid_gt"])
        assert list(ig) == g[tag + "ignored_gt"].tolist() and list(idt) == g[tag + "ignored_dt"].tolist()
        assert np.array_equal(np.asarray(dc, dtype=np.float64).reshape(-1, 4), g[tag + "dc"])
        ov = KO.image_overlap(dt["bbox"], gt["bbox"])
        for metric, mo in ((0, 0.5), (1, 0.7)):
            th = float(g[tag + "m%d.thresh" % metric])
            if impl == "oracle":
                p1 = KO.statistics(ov, gd, dd, ig, idt, dc, metric, mo, 0.0, False)
                p2 = KO.statistics(ov, gd, dd, ig, idt, dc, metric, mo, th, True, True)
            else:
                p1 = E.compute_statistics_jit(ov, gd, dd, ig, idt, dc, metric, mo)
                p2 = E.compute_statistics_jit(ov, gd, dd, ig, idt, dc, metric, mo, thresh=th, compute_fp=True, compute_aos=True)
            # pass 1 (compute_fp False): tp, fn and the true positives' scores are what eval_class uses of it
            assert [p1[0], p1[2]] == g[tag + "m%d.pass1" % metric][[0, 2]].tolist(), (tag, metric)
            assert list(p1[4]) == g[tag + "m%d.tp_scores" % metric].tolist()
            assert list(p2[:3]) == g[tag + "m%d.pass2" % metric].tolist(), (tag, metric)
            want_sim = float(g[tag + "m%d.similarity" % metric])
            if impl == "oracle":
                assert p2[3] == pytest.approx(want_sim, abs=1e-12)
            else:                    # the native pass reports "no detections" (-1) as 0: eval_class adds it only when != -1
                assert p2[3] == pytest.approx(max(want_sim, 0.0), abs=1e-12)
            n += 1
    assert n == 3 * 3 * 14 * 2
    for i in range(3):
        s, n_gt = g["thr%d.scores" % i], int(g["thr%d.num_gt" % i])
        got = KO.score_thresholds(list(s), n_gt) if impl == "oracle" else E.get_thresholds(s.copy(), n_gt)
        assert list(got) == g["thr%d.out" % i].tolist()
    if impl == "product":
        assert E.get_split_parts(10, 3) == g["split_parts.10_3"].tolist() and E.get_split_parts(9, 3) == g["split_parts.9_3"].tolist()


def test_oracle_eval_class_and_ap_match_the_reference_for_all_three_metrics():
    """precision / recall (/ orientation) arrays [class, difficulty, overlap, 41] and AP40 of the reference's eval_class on the
    12-frame set: metric 0 entirely the reference's; metrics 1, 2 the reference's host logic on the oracle's rotated
    overlaps (see the module docstring) -- so equality here pins the oracle's matching / recall sampling / AP for them and
    its 3D height-overlap arithmetic (d3_box_overlap_kernel ran as the reference wrote it)"""
    g = load_golden("f4_kitti_eval.npz")
    gts, dts = synth.random_kitti_annos(5, frames=12)
    classes = [1, 2, 0]
    mo = KO.MIN_OVERLAPS[:, :, classes]
    for metric in (0, 1, 2):
        prec, rec, aos = KO.eval_class(gts, dts, classes, (0, 1, 2), metric, mo, compute_aos=(metric == 0))
        assert np.allclose(prec, g["eval_class.m%d.precision" % metric], rtol=0, atol=1e-12), metric
        assert np.allclose(rec, g["eval_class.m%d.recall" % metric], rtol=0, atol=1e-12), metric
        if metric == 0:
            assert np.allclose(aos, g["eval_class.m0.orientation"], rtol=0, atol=1e-12)
        assert np.allclose(KO.ap40(prec), g["eval_class.m%d.ap40" % metric], rtol=0, atol=1e-9)
        assert np.any((g["eval_class.m%d.ap40" % metric] > 0) & (g["eval_class.m%d.ap40" % metric] < 100))     # non-trivial
    for crit in (-1, 0, 1):          # the 3D overlap from a given BEV intersection: reference host loop vs the oracle's
        bx, qx = g["d3.boxes"], g["d3.qboxes"]
        assert np.allclose(KO.box3d_overlap(bx, qx, crit), g["d3.out.c%d" % crit], rtol=0, atol=1e-12)
    for tag, types in (("bbox", ("bbox",)), ("all", ("bbox", "bev", "3d"))):
        res = KO.kitti_eval(gts, dts, ["Pedestrian", "Cyclist", "Car"], eval_types=types)
        keys, vals = g["kitti_eval.%s.keys" % tag].tolist(), g["kitti_eval.%s.values" % tag]
        assert sorted(res) == sorted(keys)
        for k, v in zip(keys, vals):
            assert res[k] == pytest.approx(float(v), abs=1e-9), k


def test_product_2d_evaluation_matches_the_reference_end_to_end_on_cpu():
    """kitti_eval(eval_types=['bbox']) of the product (native matching library, no device) vs the reference's own run:
    every AP number and the printed table"""
    from engine.kitti_eval import kitti_eval
    g = load_golden("f4_kitti_eval.npz")
    gts, dts = synth.random_kitti_annos(5, frames=12)
    text, res = kitti_eval(gts, dts, ["Pedestrian", "Cyclist", "Car"], eval_types=["bbox"])
    keys, vals = g["kitti_eval.bbox.keys"].tolist(), g["kitti_eval.bbox.values"]
    assert list(res.keys()) == keys                       # same keys in the same order
    for k, v in zip(keys, vals):
        assert res[k] == pytest.approx(float(v), abs=1e-9), k
    assert text == bytes(g["kitti_eval.bbox.text"]).decode()


@pytest.mark.gpu
def test_product_full_evaluation_matches_the_reference_host_logic_on_gpu():
    """all three metrics through the HIP overlap kernels + native matching vs the reference's evaluator (whose rotated
    overlaps came from the oracle: float32 formulations differ by round-off, so AP to 1e-6, the table line by line after
    rounding as the reference prints it)"""
    from engine.kitti_eval import kitti_eval
    g = load_golden("f4_kitti_eval.npz")
    gts, dts = synth.random_kitti_annos(5, frames=12)
    text, res = kitti_eval(gts, dts, ["Pedestrian", "Cyclist", "Car"], eval_types=["bbox", "bev", "3d"])
    keys, vals = g["kitti_eval.all.keys"].tolist(), g["kitti_eval.all.values"]
    assert list(res.keys()) == keys
    for k, v in zip(keys, vals):
        assert res[k] == pytest.approx(float(v), abs=1e-6), k
    assert text == bytes(g["kitti_eval.all.text"]).decode()


@pytest.mark.gpu
def test_gpu_preprocess_is_the_reference_transform_chain():
    """mc_preprocess (uint8 / float32 HWC frames -> normalised, padded NCHW batch) vs the reference's Normalize -> Pad ->
    ToTensor output directly (not through the oracle)"""
    from hipmonocon.engine import Engine
    g = load_golden("f4_transforms.npz")
    eng = Engine()
    for dt in ("uint8", "float32"):
        for i, (h, w) in enumerate(SIZES):
            batch, pads = eng.preprocess([torch.from_numpy(_frame(i, h, w, dt)).cuda()])
            tag = "%dx%d.%s." % (h, w, dt)
            assert list(pads[0]) == g[tag + "pad_shape"].tolist()
            _check_img(g, tag, batch[0].cpu())
