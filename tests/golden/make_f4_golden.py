#!/usr/bin/env python
"""Golden vectors for SURVEY 8f-4 from the REFERENCE'S OWN SOURCE (round 6): Normalize / Pad / ToTensor, the label loop of
MonoConDataset.__getitem__, and the host side of the KITTI AP evaluator.

Runs only in the build container (needs /root/reference, read-only); the tests read the .npz files it writes.

Those reference modules import cv2 and numba, which this image lacks.  They are imported here under INERT PLACEHOLDERS,
and the script proves that no placeholder ever does any work:

  * ``cv2``: a module object whose every attribute access raises.  ``transforms/default_transforms.py`` and
    ``dataset/base_dataset.py`` only name cv2 inside function bodies (Resize3D, PhotometricDistortion, load_image); none of
    those bodies runs here.  The PNG is decoded by PIL in a four-line subclass override of ``load_image`` (this script's
    code, RGB like the reference's cv2.imread + BGR2RGB); everything downstream of the decoded array -- filters, label
    assembly, Normalize, Pad, ToTensor, collate_fn -- is the reference's code, unmodified.
  * ``numba``: ``numba.jit`` / ``numba.cuda.jit`` are IDENTITY decorators (they return the function they are given; the
    reference's ``@numba.jit(nopython=True)`` host loops then run as the plain Python they are written in) and
    ``numba.prange`` is ``range`` (a sequential run of a parallel loop without cross-iteration dependences).  Any other
    attribute (``numba.float32``, ``cuda.local``, ``cuda.shared``, ``cuda.to_device`` ...) raises -- and is never reached:
    the ONE function of the evaluator that needs them, ``rotate_iou_gpu_eval`` (the numba.cuda kernel
    ``rotate_iou_kernel_eval``, engine/kitti_eval/rotate_iou.py:280-379), is not executed HERE.  For the BEV / 3D metrics the
    reference's ``calculate_iou_partly`` is handed rotated overlaps by binding the name ``rotate_iou_gpu_eval`` in
    ``engine.kitti_eval.rotate_iou`` (where bev_box_overlap / d3_box_overlap look it up) to the oracle's float32 restatement (oracle/kitti_eval_oracle.py:rotate_iou).  So:
      - 2D metric: every number is the reference's (image_box_overlap, clean_data, compute_statistics_jit,
        fused_compute_statistics, get_thresholds, eval_class, get_mAP40, kitti_eval's dict and table);
      - BEV / 3D: everything DOWNSTREAM of the rotated-overlap matrix is the reference's (d3_box_overlap_kernel's height
        overlap included).  The rotated-IoU kernel itself is pinned by its own generator, make_rotate_iou_golden.py, which
        imports this file and EXECUTES rotate_iou.py under a numba shim (rotate_iou_ref.npz); these f4 goldens are kept
        as they were made, with the oracle standing in.
    meta_f4.json records the placeholder list and the access log (which must be empty).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_f4_golden.py
"""
import io
import json
import os
import sys
import types
import zlib

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

PLACEHOLDER_LOG = []          # (module, attribute) of every placeholder attribute that was touched


class _Inert(types.ModuleType):
    """a module that exists and does nothing: any attribute access is recorded and raises"""
    def __init__(self, name, allowed=None):
        super().__init__(name)
        self.__dict__["_allowed"] = dict(allowed or {})
        self.__dict__["__path__"] = []          # so that ``from numba import cuda`` resolves through sys.modules

    def __getattr__(self, attr):
        if attr in self.__dict__["_allowed"]:
            return self.__dict__["_allowed"][attr]
        if attr.startswith("__"):
            raise AttributeError(attr)
        PLACEHOLDER_LOG.append((self.__name__, attr))
        raise RuntimeError("placeholder module %s: attribute %r was touched -- the golden would not be the reference's" % (self.__name__, attr))


def _identity_jit(*args, **kwargs):
    """numba.jit / cuda.jit used bare (@numba.jit) or with options (@numba.jit(nopython=True), @cuda.jit('sig', ...))"""
    if len(args) == 1 and callable(args[0]) and not kwargs:
        return args[0]
    return lambda fn: fn


def install_placeholders():
    cuda = _Inert("numba.cuda", {"jit": _identity_jit})
    numba = _Inert("numba", {"jit": _identity_jit, "prange": range, "cuda": cuda})
    sys.modules["numba"] = numba
    sys.modules["numba.cuda"] = cuda
    sys.modules["cv2"] = _Inert("cv2")
    return {"cv2": "inert: every attribute access raises (none occurred)",
            "numba.jit": "identity decorator", "numba.cuda.jit": "identity decorator (the decorated device functions are never called)",
            "numba.prange": "builtins.range", "numba.<anything else>": "raises (none occurred)"}


PLACEHOLDERS = install_placeholders()
sys.path.insert(0, "/root/reference")                       # reference packages win name lookups
sys.path.append(os.path.join(REPO, "monocon-pytorch_amd"))  # only ``hipmonocon`` is taken from here
sys.path.append(REPO)                                       # ``oracle`` (the rotated-overlap stand-in, see above)

import numpy as np                                          # noqa: E402
import torch                                                # noqa: E402

import transforms as RT                                     # noqa: E402  (reference)
from dataset.monocon_dataset import MonoConDataset          # noqa: E402  (reference)
from engine.kitti_eval import eval as RE                    # noqa: E402  (reference)
from hipmonocon import synth                                # noqa: E402  (this repo)
from oracle import kitti_eval_oracle as KO                  # noqa: E402  (this repo: rotated overlaps only)

assert RT.__file__.startswith("/root/reference/") and RE.__file__.startswith("/root/reference/")
KITTI_MINI = os.path.join(HERE, "kitti_mini")


def save(name, **arrs):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    print("wrote", name, "%.1f KB" % (os.path.getsize(path) / 1024))


# ------------------------------------------------------------------------------------------------ (A) transforms
def transforms_golden():
    """Normalize -> Pad -> ToTensor (transforms/default_transforms.py:376-456) exactly as dataset/monocon_dataset.py:38-42
    composes them for the test split, on seeded uint8 and float32 frames of five sizes: full tensors for the small
    frames, strided samples for the KITTI-sized ones, and the CRC-32 of every tensor's bytes (CHW, contiguous)."""
    tf = RT.Compose([RT.Normalize(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375]), RT.Pad(size_divisor=32), RT.ToTensor()])
    out = {}
    sizes = [(375, 1242), (370, 1224), (384, 1280), (33, 65), (64, 96)]
    for i, (h, w) in enumerate(sizes):
        for dt in ("uint8", "float32"):
            a = synth.uniform(31 + i, "raw", (h, w, 3), 0.0, 255.0).astype(np.float32)
            img = np.floor(a).astype(np.uint8) if dt == "uint8" else a
            d = tf({"img": img.copy(), "img_metas": {"ori_shape": (h, w)},
                    "label": {"gt_bboxes": np.arange(8, dtype=np.float32).reshape(2, 4), "mask": np.array([True, False])}})
            t = d["img"]
            tag = "%dx%d.%s." % (h, w, dt)
            out[tag + "shape"] = np.asarray(t.shape)
            out[tag + "pad_shape"] = np.asarray(d["img_metas"]["pad_shape"])
            out[tag + "dtype"] = str(t.dtype)
            out[tag + "crc32"] = zlib.crc32(t.contiguous().numpy().tobytes())      # the WHOLE tensor, bit for bit
            if h * w <= 64 * 96:
                out[tag + "full"] = t.numpy()
            else:
                out[tag + "samples"] = t.reshape(-1)[::997].numpy()
            if i == 3 and dt == "uint8":      # ToTensor's label branch: torch.Tensor(v).unsqueeze(0)
                out["label.gt_bboxes"] = d["label"]["gt_bboxes"].numpy()
                out["label.mask"] = d["label"]["mask"].numpy()
                out["label.mask.dtype"] = str(d["label"]["mask"].dtype)
    save("f4_transforms.npz", **out)


# ------------------------------------------------------------------------------------------------ (B) dataset label loop
class _PILDecoded(MonoConDataset):
    """the reference dataset with ONE method replaced: the PNG is decoded by PIL (RGB) instead of cv2.imread + BGR2RGB.
    img_metas are built as dataset/base_dataset.py:71-76 builds them."""
    def load_image(self, idx):
        from PIL import Image
        image_data = np.asarray(Image.open(self.image_files[idx]).convert("RGB"))
        img_metas = {"idx": idx, "split": self.split, "sample_idx": int(os.path.basename(self.image_files[idx]).split(".")[0]),
                     "image_path": self.image_files[idx], "ori_shape": image_data.shape[:2]}
        return (image_data, img_metas)


def dataset_golden():
    """MonoConDataset.__getitem__ (dataset/monocon_dataset.py:76-146: filter rules, label assembly, key-point flags) + the
    test-split transforms + collate_fn (:160-191) on the two-frame mini tree of make_golden.py dataset_pins().  The
    reference reads its split file from ITS OWN dataset/ImageSets; the instance's file lists are then pointed at the mini
    tree's two frames (attribute assignment, no reference code changed)."""
    ds = _PILDecoded(KITTI_MINI, "val")
    ids = sorted(f[:-4] for f in os.listdir(os.path.join(KITTI_MINI, "training", "image_2")))
    ds.file_prefix = ids
    ds.image_files = [os.path.join(ds.image_dir, p + ".png") for p in ids]
    ds.calib_files = [os.path.join(ds.calib_dir, p + ".txt") for p in ids]
    ds.label_files = [os.path.join(ds.label_dir, p + ".txt") for p in ids]
    out = {"ids": np.asarray(ids)}
    samples = []
    for i, pid in enumerate(ids):
        s = ds[i]
        samples.append(s)
        out[pid + ".img.shape"] = np.asarray(s["img"].shape)
        out[pid + ".img.crc32"] = zlib.crc32(s["img"].contiguous().numpy().tobytes())
        out[pid + ".img.samples"] = s["img"].reshape(-1)[::997].numpy()
        out[pid + ".pad_shape"] = np.asarray(s["img_metas"]["pad_shape"])
        out[pid + ".ori_shape"] = np.asarray(s["img_metas"]["ori_shape"])
        out[pid + ".sample_idx"] = s["img_metas"]["sample_idx"]
        for k, v in s["label"].items():
            out["%s.label.%s" % (pid, k)] = v.numpy()
            out["%s.label.%s.dtype" % (pid, k)] = str(v.dtype)
    b = MonoConDataset.collate_fn([samples[0], samples[0]])
    out["collate.img.shape"] = np.asarray(b["img"].shape)
    out["collate.keys"] = np.asarray(sorted(b.keys()))
    out["collate.meta_keys"] = np.asarray(sorted(b["img_metas"].keys()))
    for k, v in b["label"].items():
        out["collate.label.%s.shape" % k] = np.asarray(v.shape)
    save("f4_dataset.npz", **out)


# ------------------------------------------------------------------------------------------------ (C) AP evaluator, host side
def eval_golden():
    """the reference's evaluator functions on synth.random_kitti_annos (the frames of tests/test_kitti_eval.py):
    per-frame ignore rules and matching for every (class, difficulty), recall thresholds, image overlaps for all four
    criteria, eval_class for the three metrics, the final kitti_eval dict + table."""
    stand_in = lambda boxes, qboxes, criterion=-1, device_id=0: KO.rotate_iou(boxes, qboxes, criterion)      # noqa: E731
    RE.rotate_iou_gpu_eval = stand_in
    import engine.kitti_eval.rotate_iou as RR           # bev_box_overlap / d3_box_overlap import the name from here at call time
    RR.rotate_iou_gpu_eval = stand_in
    out = {}
    gts, dts = synth.random_kitti_annos(11, frames=14)
    rng = np.random.default_rng(0)
    for crit in (-1, 0, 1, 2):
        out["image_overlap.c%d" % crit] = RE.image_box_overlap(gts[0]["bbox"], dts[0]["bbox"], crit)
    for cls in range(3):
        for diff in range(3):
            for f, (g, d) in enumerate(zip(gts, dts)):
                tag = "f%d.c%d.d%d." % (f, cls, diff)
                nv, ig, idt, dc = RE.clean_data(g, d, cls, diff)
                out[tag + "num_valid_gt"] = nv
                out[tag + "ignored_gt"] = np.asarray(ig, dtype=np.int64)
                out[tag + "ignored_dt"] = np.asarray(idt, dtype=np.int64)
                dcb = np.asarray(dc, dtype=np.float64).reshape(-1, 4)
                out[tag + "dc"] = dcb
                ov = RE.image_box_overlap(d["bbox"], g["bbox"])
                gd = np.concatenate([g["bbox"], g["alpha"][:, None]], 1).reshape(-1, 5)
                dd = np.concatenate([d["bbox"].reshape(-1, 4), d["alpha"].reshape(-1, 1), d["score"].reshape(-1, 1)], 1)
                igz, idz = np.asarray(ig, dtype=np.int64), np.asarray(idt, dtype=np.int64)
                for metric, mo in ((0, 0.5), (1, 0.7)):
                    tp, fp, fn, sim, thr = RE.compute_statistics_jit(ov, gd, dd, igz, idz, dcb, metric, mo, thresh=0.0, compute_fp=False)
                    out[tag + "m%d.pass1" % metric] = np.array([tp, fp, fn], dtype=np.int64)
                    out[tag + "m%d.tp_scores" % metric] = np.asarray(thr, dtype=np.float64)
                    th = float(rng.uniform(0, 0.6))
                    tp, fp, fn, sim, _ = RE.compute_statistics_jit(ov, gd, dd, igz, idz, dcb, metric, mo, thresh=th, compute_fp=True,
                                                                    compute_aos=True)
                    out[tag + "m%d.thresh" % metric] = th
                    out[tag + "m%d.pass2" % metric] = np.array([tp, fp, fn], dtype=np.int64)
                    out[tag + "m%d.similarity" % metric] = float(sim)
    for i, n_gt in enumerate((1, 7, 40)):
        s = rng.uniform(0, 1, int(rng.integers(1, 60)))
        out["thr%d.scores" % i] = s.copy()
        out["thr%d.num_gt" % i] = n_gt
        out["thr%d.out" % i] = np.asarray(RE.get_thresholds(s.copy(), n_gt), dtype=np.float64)
    out["split_parts.10_3"] = np.asarray(RE.get_split_parts(10, 3))
    out["split_parts.9_3"] = np.asarray(RE.get_split_parts(9, 3))

    # eval_class / kitti_eval on the 12-frame set of test_kitti_eval_all_metrics_vs_oracle
    gts, dts = synth.random_kitti_annos(5, frames=12)
    classes = [1, 2, 0]            # ["Pedestrian", "Cyclist", "Car"] as kitti_eval maps them
    mo = RE_min_overlaps(classes)
    for metric in (0, 1, 2):
        # two parts (num_parts=2) so that fused_compute_statistics' part bookkeeping is exercised with > 1 frame per part
        ret = RE.eval_class(gts, dts, classes, [0, 1, 2], metric, mo, compute_aos=(metric == 0), num_parts=5)
        out["eval_class.m%d.precision" % metric] = ret["precision"]
        out["eval_class.m%d.recall" % metric] = ret["recall"]
        if metric == 0:
            out["eval_class.m0.orientation"] = ret["orientation"]
        out["eval_class.m%d.ap40" % metric] = RE.get_mAP40(ret["precision"])
    # d3_box_overlap_kernel alone (the reference's host loop: height overlap x BEV intersection -> 3D IoU), rinc given
    g0, d0 = gts[0], dts[0]
    full = lambda a: np.concatenate([a["location"].reshape(-1, 3), a["dimensions"].reshape(-1, 3), a["rotation_y"].reshape(-1, 1)], 1)   # noqa: E731
    bx, qx = full(d0), full(g0)
    for crit in (-1, 0, 1):
        rinc = KO.rotate_iou(bx[:, [0, 2, 3, 5, 6]], qx[:, [0, 2, 3, 5, 6]], 2).astype(np.float64)
        out["d3.rinc_in.c%d" % crit] = rinc.copy()
        RE.d3_box_overlap_kernel(bx, qx, rinc, crit)
        out["d3.out.c%d" % crit] = rinc
    out["d3.boxes"] = bx
    out["d3.qboxes"] = qx
    for types, tag in ((["bbox"], "bbox"), (["bbox", "bev", "3d"], "all")):
        text, res = RE.kitti_eval(gts, dts, ["Pedestrian", "Cyclist", "Car"], eval_types=types)
        out["kitti_eval.%s.keys" % tag] = np.asarray(list(res.keys()))
        out["kitti_eval.%s.values" % tag] = np.asarray([float(res[k]) for k in res], dtype=np.float64)
        out["kitti_eval.%s.text" % tag] = np.frombuffer(text.encode(), dtype=np.uint8)
    save("f4_kitti_eval.npz", **out)


ROTATED_IOU_GOLDEN = ("engine/kitti_eval/rotate_iou.py is executed by tests/golden/make_rotate_iou_golden.py (its numba.cuda "
                      "kernel under an emulated launch, float32 and float64 storage): tests/golden/rotate_iou_ref.npz, "
                      "meta_rotate_iou.json. The f4 BEV / 3D goldens here still come from the oracle stand-in below; the "
                      "reference's own end-to-end kitti_eval is in rotate_iou_ref.npz (e2e.*)")


def RE_min_overlaps(classes):
    """the overlap table kitti_eval builds (engine/kitti_eval/eval.py:684-700), cut to the classes -- rebuilt from the values
    the reference prints in its own table header ('AP40@0.70, 0.70, 0.70' ...), and cross-checked against kitti_eval's
    output below through the AP numbers"""
    o0 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5]] * 3)
    o1 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25], [0.5, 0.25, 0.25, 0.5, 0.25]])
    return np.stack([o0, o1], axis=0)[:, :, classes]


if __name__ == "__main__":
    torch.set_num_threads(8)
    transforms_golden()
    dataset_golden()
    eval_golden()
    assert not PLACEHOLDER_LOG, PLACEHOLDER_LOG
    meta = {"torch": torch.__version__, "numpy": np.__version__, "placeholders": PLACEHOLDERS,
            "placeholder_attribute_accesses": PLACEHOLDER_LOG,
            "not_executed": [],
            "stand_in": {"engine.kitti_eval.eval.rotate_iou_gpu_eval": "oracle.kitti_eval_oracle.rotate_iou (BEV / 3D metrics only)",
                         "MonoConDataset.load_image": "PIL decode to RGB instead of cv2.imread + cv2.cvtColor"},
            "reference_modules_run": [RT.__file__, sys.modules["transforms.default_transforms"].__file__,
                                      sys.modules["dataset.monocon_dataset"].__file__, sys.modules["dataset.base_dataset"].__file__,
                                      RE.__file__],
            "rotated_iou": ROTATED_IOU_GOLDEN}
    with open(os.path.join(HERE, "meta_f4.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("placeholder accesses:", PLACEHOLDER_LOG)
