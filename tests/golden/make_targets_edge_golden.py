#!/usr/bin/env python
"""tests/golden/targets_edge.npz: the REAL reference's TargetGenerator and MonoConDenseHeads._get_losses on the label
shapes KITTI training produces after RandomShift / RandomCrop3D / RandomHorizontalFlip and synth.make_labels never draws:
masks with holes (poison in the unmasked slots), an empty image inside a batch, objects whose nine keypoints are all
invisible or off the map, several objects on one pixel, centres in the border pixels with radius 0 and with a radius that
crosses two borders, boxes on which an fp32 and a double evaluation of gaussian_radius floor to different integers, and
angles outside (-pi, pi] and next to the bin boundaries.

Groups (every key is "<group>.<name>"):
    edge       6 images at 192x384 -> 48x96: 0 mask holes + poison, 1 empty, 2 all keypoints dead, 3 shared pixels,
               4 border centres, 5 radius-boundary boxes + angles
    dead       2 images whose keypoints are all invisible (valid == 0) or visible but off the map
    invisible  2 images whose keypoints all have valid == 0 (loss_center2kpt_offset is exactly 0)
    kitti      1 image at 384x1280 -> 96x320 with the three radius-boundary boxes named in radius_boxes_kitti
per group: in.* (the label inputs, the single source of the inputs), the 15 targets, exp.* (every fp32 Tensor.exp call
of the target generator, as in targets_exp.npz), pred.seed (the prediction maps are synth.make_decode_inputs(seed, B, fh,
fw) with the flat entries clamp_lo.<map> / clamp_hi.<map> of the two heat-maps set to fp32(1e-4) / fp32(1 - 1e-4);
n_on_clamp.<map> = [low, high] counts them on the final maps), loss32.* / loss64.* (the ten losses on fp32 / fp64 maps),
and for the gradient of sum_i w_i loss_i (w = loss_weights) with respect to each map, in fp32 (g32) and fp64 (g64):
gnorm, gsample (stride max(1, numel // 2048)) and, for the eight regression maps, nz (flat indices of every non-zero
entry) with nzval.  radius.hw / radius.ref / radius.double: (h, w) pairs with the reference's and a double evaluation's
floored radius, the disagreeing ones first.

Needs a checkout of the reference project (its path is the argument); the tests read only the .npz.
Host dependence: center_heatmap_target and kpt_heatmap_target hold fp32 exp results (torch's CPU exp goes through a vector
math library that dispatches by CPU), so their last bit -- and with it the low bits of the two focal losses and of the
heat-map gradients -- may move on another host; everything else is reproduced byte for byte.  The exp table makes the CPU
test independent of that.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_targets_edge_golden.py <reference checkout>
"""
import math
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.abspath(sys.argv[1]))           # reference packages win name lookups
sys.path.append(os.path.join(REPO, "monocon-pytorch_amd"))

import numpy as np
import torch
from utils.target_generator import TargetGenerator          # noqa: E402  (reference)
from utils.tensor_ops import gaussian_radius as ref_radius   # noqa: E402  (reference)
from model import MonoConDenseHeads                         # noqa: E402  (reference)
from hipmonocon import synth                                # noqa: E402  (this repo)

torch.set_num_threads(8)
SEED = 7
H, W = 192, 384
PI = math.pi
F32 = np.float32
LOSS_WEIGHTS = np.array([1.0, 0.5, 2.0, 1.5, 1.0, 0.7, 1.0, 3.0, 1.0, 0.25], np.float32)   # test_loss_gradients_vs_autograd
HEAT = ("center_heatmap_pred", "kpt_heatmap_pred")
LO, HI = F32(1e-4), F32(1 - 1e-4)
BOUNDARY_BINS = (1, 6, 12, -3)
# three boxes [x1, y1, x2, y2] found in the first report of the disagreement, at 384x1280, stride 4: reference radius, double-evaluated radius
KITTI_BOXES = [([251.7559356689453, 231.15426635742188, 358.4798583984375, 383.0], 7, 6),
               ([1125.3323974609375, 29.458070755004883, 1252.580810546875, 100.57401275634766], 5, 4),
               ([584.727783203125, 218.52171325683594, 832.7520141601562, 383.0], 11, 10)]


# ------------------------------------------------------------------------------------------------ radius
def radius_double(h, w, mo=0.3):
    h, w = float(h), float(w)
    b1 = h + w
    r1 = (b1 - math.sqrt(b1 * b1 - 4 * (w * h * (1 - mo) / (1 + mo)))) / 2
    b2 = 2 * (h + w)
    r2 = (b2 - math.sqrt(b2 * b2 - 16 * ((1 - mo) * w * h))) / 8
    a3, b3, c3 = 4 * mo, -2 * mo * (h + w), (mo - 1) * w * h
    r3 = (b3 + math.sqrt(b3 * b3 - 4 * a3 * c3)) / (2 * a3)
    return max(0, int(min(r1, r2, r3)))


def radius_reference(h, w):
    """the reference's own call, on 0-dim fp32 tensors as TargetGenerator passes them"""
    return max(0, int(ref_radius((torch.tensor(h, dtype=torch.float32), torch.tensor(w, dtype=torch.float32)))))


def radius_models(h, w):
    """vectorised fp32 and double evaluations (numpy), used only to FIND candidates"""
    out = []
    for dt in (np.float32, np.float64):
        hh, ww = h.astype(dt), w.astype(dt)
        c = lambda v: dt(v)                                                           # noqa: E731
        sq = lambda v: np.sqrt(v.astype(np.float64)).astype(dt)                        # noqa: E731
        b1 = hh + ww
        r1 = (b1 - sq(b1 * b1 - c(4) * (ww * hh * c(0.7) / c(1.3)))) / c(2)
        b2 = c(2) * (hh + ww)
        r2 = (b2 - sq(b2 * b2 - c(16) * (c(0.7) * ww * hh))) / c(8)
        b3 = c(-0.6) * (hh + ww)
        r3 = (b3 + sq(b3 * b3 - c(4.8) * (c(-0.7) * ww * hh))) / c(2.4)
        out.append(np.floor(np.minimum(r1, np.minimum(r2, r3))))
    return out


def find_radius_boundary_boxes(want=4):
    """seeded search over boxes inside the 192x384 image; every hit is confirmed against the reference's gaussian_radius"""
    rng = np.random.default_rng(20240607)
    found = []
    for _ in range(200):
        n = 2_000_000
        x1 = rng.uniform(0, W - 30, n).astype(F32)
        y1 = rng.uniform(0, H - 30, n).astype(F32)
        x2 = np.minimum(x1 + rng.uniform(24, 256, n).astype(F32), F32(W - 1)).astype(F32)
        y2 = np.minimum(y1 + rng.uniform(24, 160, n).astype(F32), F32(H - 1)).astype(F32)
        bh = ((y2 - y1) * F32(0.25)).astype(F32)
        bw = ((x2 - x1) * F32(0.25)).astype(F32)
        r32, r64 = radius_models(bh, bw)
        for i in np.nonzero(r32 != r64)[0]:
            a, b = radius_reference(bh[i], bw[i]), radius_double(bh[i], bw[i])
            if a != b:
                found.append((np.array([x1[i], y1[i], x2[i], y2[i]], F32), a, b))
        if len(found) >= want:
            break
    assert len(found) >= 3, "found only %d radius-boundary boxes" % len(found)
    return found[:want]


# ------------------------------------------------------------------------------------------------ labels
def set_obj(lab, b, s, box=None, cls=None, yaw=None, kpts=None, valid=None):
    if box is not None:
        lab["gt_bboxes"][b, s] = np.asarray(box, F32)
        lab["centers2d"][b, s] = [(box[0] + box[2]) / 2, (box[1] + box[3]) / 2]
    if cls is not None:
        lab["gt_labels"][b, s] = lab["gt_labels_3d"][b, s] = cls
    if yaw is not None:
        lab["gt_bboxes_3d"][b, s, 6] = yaw
    if kpts is not None:
        lab["gt_kpts_2d"][b, s] = np.asarray(kpts, F32).reshape(-1)
    if valid is not None:
        lab["gt_kpts_valid_mask"][b, s] = np.asarray(valid, F32)


def poison(lab, b, s):
    lab["gt_bboxes"][b, s] = np.nan
    lab["gt_labels"][b, s] = lab["gt_labels_3d"][b, s] = 7
    lab["centers2d"][b, s] = [1e6, -1e6]
    lab["gt_bboxes_3d"][b, s] = np.nan
    lab["depths"][b, s] = np.nan
    lab["gt_kpts_2d"][b, s] = np.nan
    lab["gt_kpts_valid_mask"][b, s] = 2


OFF_MAP = [(-8.0, 50.0), (W + 4.0, 60.0), (100.0, -8.0), (120.0, H + 4.0),      # left, right, top, bottom
           (float(W), 70.0), (130.0, float(H)), (-4.0, -4.0), (W + 40.0, H + 40.0), (-400.0, 90.0)]


def kill_keypoints(lab, b, s, style):
    """style 0: valid == 0 for all nine; 1: all visible but off the map (each of the four sides, the first coordinate past
    the map, corners); 2: a mix of both"""
    if style == 0:
        lab["gt_kpts_valid_mask"][b, s] = 0
    elif style == 1:
        set_obj(lab, b, s, kpts=OFF_MAP, valid=[1, 2, 1, 2, 1, 2, 1, 2, 1])
    else:
        set_obj(lab, b, s, kpts=OFF_MAP, valid=[1, 0, 2, 0, 1, 0, 0, 2, 1])


def angle_list():
    """(angles, dropped): the explicit values and the fp32 neighbours (-3 .. +1 ulp: the fp32 modulo and add move the
    switch by up to two) of the bin boundaries k * pi/6 - pi/12; an angle on which
    the reference does not return a class in 0..11 (or trips its own range assertion) is dropped and printed"""
    vals = [0.0, -0.0, PI, -PI, 2 * PI, -2 * PI, 2 * PI + 0.3, 4 * PI]
    for k in BOUNDARY_BINS:
        f = F32(k * PI / 6 - PI / 12)
        down = [f]
        for _ in range(3):
            down.append(np.nextafter(down[-1], F32(-np.inf)))
        vals += [float(v) for v in down[:0:-1]] + [float(f), float(np.nextafter(f, F32(np.inf)))]      # -3 .. +1 ulp
    tg = TargetGenerator()
    keep, dropped = [], []
    for v in vals:
        try:
            cid, _ = tg._convert_angle_to_class(torch.tensor(v, dtype=torch.float32))
            ok = 0 <= cid <= 11
        except AssertionError:
            ok = False
        (keep if ok else dropped).append(v)
    for v in dropped:
        print("angle %r dropped: the reference returns no class in 0..11 for it" % v)
    return np.array(keep, F32), dropped


def edge_labels(rboxes, angles):
    lab = synth.make_labels(SEED + 20, 6, H, W, min_objs=30, max_gen=30)      # every slot starts with finite values
    lab["mask"][:] = 0
    # image 0: mask holes {0, 2, 5}, poison in the unmasked slots between, stale finite values behind
    lab["mask"][0, [0, 2, 5]] = 1
    for s in (1, 3, 4):
        poison(lab, 0, s)
    # image 1: no object (stale finite values in every slot)
    # image 2: five objects, every keypoint dead
    lab["mask"][2, :5] = 1
    for s, style in enumerate((0, 1, 2, 1, 0)):
        kill_keypoints(lab, 2, s, style)
    # image 3: shared pixels
    lab["mask"][3, :9] = 1
    for s, (cx, cy, bw, bh) in enumerate([(160.5, 80.5, 16.0, 12.0), (161.7, 82.2, 48.0, 60.0), (163.9, 83.9, 100.0, 30.0),
                                          (162.0, 81.0, 200.0, 150.0)]):
        set_obj(lab, 3, s, box=[cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], cls=0)      # pixel (40, 20), one class
    lab["depths"][3, :4] = [2.5, 9.0, 33.0, 64.0]
    lab["gt_bboxes_3d"][3, :4, 2] = lab["depths"][3, :4]
    lab["gt_bboxes_3d"][3, :4, 3:6] = [[0.4, 0.5, 0.3], [1.2, 1.6, 0.9], [2.5, 1.7, 1.6], [6.0, 3.0, 2.6]]
    set_obj(lab, 3, 4, box=[262.0, 100.0, 302.0, 144.0], cls=1)                                  # pixel (70, 30), class 1
    set_obj(lab, 3, 5, box=[250.1, 90.3, 316.9, 156.7], cls=2)                                   # pixel (70, 30), class 2
    k6 = lab["gt_kpts_2d"][3, 6].reshape(9, 2).copy()
    k6[0] = [-2.0, -1.0]             # scaled (-0.5, -0.25): .int() truncates to (0, 0) -> inside, a LIVE gather of pixel 0
    k6[1] = [-3.9, 100.0]            # scaled x in (-1, 0) on another row
    k6[2] = [1.0, 2.5]               # pixel 0 again, from inside
    set_obj(lab, 3, 6, kpts=k6, valid=[1, 2, 1, 1, 2, 1, 1, 2, 1])
    kill_keypoints(lab, 3, 7, 0)     # dead gathers of pixel 0 beside the live ones
    kill_keypoints(lab, 3, 8, 2)
    # image 4: border centres, each with radius 0 (a 2 px box) and with a radius that crosses two borders (a 1280 px box:
    # radius 72 > 47, so every splat is clipped on at least three sides), + one box reaching the last row and column
    border = [(0, 0), (95, 0), (0, 47), (95, 47), (10, 0), (85, 47), (0, 10), (95, 37)]
    s = 0
    for px, py in border:
        cx, cy = 4.0 * px + 2.0, 4.0 * py + 2.0
        set_obj(lab, 4, s, box=[cx - 1, cy - 1, cx + 1, cy + 1], cls=s % 3)
        set_obj(lab, 4, s + 1, box=[cx - 640, cy - 640, cx + 640, cy + 640], cls=(s + 1) % 3)
        s += 2
    for px, py in border[:4]:       # a moderate radius (36) too: clipped on two sides only
        cx, cy = 4.0 * px + 1.0, 4.0 * py + 3.0
        set_obj(lab, 4, s, box=[cx - 320, cy - 320, cx + 320, cy + 320], cls=s % 3)
        s += 1
    set_obj(lab, 4, s, box=[W - 40.0, H - 30.0, W - 0.01, H - 0.01], cls=0)
    lab["mask"][4, :s + 1] = 1
    # image 5: radius-boundary boxes first, then synthetic boxes; the angle list over the slots
    for i, (box, _, _) in enumerate(rboxes):
        set_obj(lab, 5, i, box=box)
    assert len(angles) <= 30
    for i, a in enumerate(angles):
        lab["gt_bboxes_3d"][5, i, 6] = a
    lab["mask"][5, :max(len(angles), len(rboxes))] = 1
    return lab


def dead_labels(seed, all_invisible):
    lab = synth.make_labels(seed, 2, H, W, min_objs=4, max_gen=6)
    for b in range(2):
        for s in range(30):
            kill_keypoints(lab, b, s, 0 if all_invisible else (s + b) % 3)
    return lab


def kitti_labels():
    lab = synth.make_labels(SEED + 23, 1, 384, 1280, min_objs=5, max_gen=5)
    for i, (box, _, _) in enumerate(KITTI_BOXES):
        set_obj(lab, 0, i, box=box)
    return lab


# ------------------------------------------------------------------------------------------------ recording
def make_preds(seed, B, fh, fw, T):
    """synth.make_decode_inputs + entries exactly on both clamp values in the two heat-maps (on positives of the target
    and elsewhere); returns (maps, {clamp_lo.<map>, clamp_hi.<map>, n_on_clamp.<map>})"""
    d = synth.make_decode_inputs(seed, B, fh, fw)
    extra = {}
    for key, tkey in zip(HEAT, ("center_heatmap_target", "kpt_heatmap_target")):
        n = d[key].size
        pos = np.nonzero(T[tkey].numpy().reshape(-1) == 1.0)[0]
        lo = np.unique(np.concatenate([synth.integers(seed, "clamp.lo." + key, (24,), 0, n), pos[0::4][:6]]))
        hi = np.unique(np.concatenate([synth.integers(seed, "clamp.hi." + key, (24,), 0, n), pos[1::4][:6]]))
        hi = np.setdiff1d(hi, lo)
        flat = d[key].reshape(-1)
        flat[lo] = LO
        flat[hi] = HI
        extra["clamp_lo." + key], extra["clamp_hi." + key] = lo.astype(np.int64), hi.astype(np.int64)
        extra["n_on_clamp." + key] = np.array([(flat == LO).sum(), (flat == HI).sum()], np.int64)
        assert extra["n_on_clamp." + key].min() >= 24
    return d, extra


def record_group(name, lab, hw, pred_seed, head):
    h, w = hw
    B = lab["mask"].shape[0]
    fh, fw = h // 4, w // 4
    calls = []
    real_exp = torch.Tensor.exp

    def recording_exp(x):
        y = real_exp(x)
        a = x.detach().numpy().copy()
        if not any(c[0].shape == a.shape and np.array_equal(c[0].view(np.uint32), a.view(np.uint32)) for c in calls):
            calls.append((a, y.detach().numpy().copy()))
        return y

    torch.Tensor.exp = recording_exp
    try:
        data = {"img": torch.zeros(B, 3, h, w), "img_metas": {"pad_shape": [(h, w)] * B},
                "label": {k: torch.from_numpy(v.copy()) for k, v in lab.items()}}
        T = TargetGenerator()(data, feat_shape=(B, 64, fh, fw))
    finally:
        torch.Tensor.exp = real_exp
    for k, v in data["label"].items():                   # the reference left its input alone
        assert np.array_equal(v.numpy(), lab[k], equal_nan=True), k
    out = {"in." + k: v for k, v in lab.items()}
    out["shape"] = np.array([B, h, w], np.int64)
    out.update({k: v.numpy() for k, v in T.items()})
    out["exp.n"] = np.int64(len(calls))
    for i, (a, y) in enumerate(calls):
        out["exp.arg%d" % i], out["exp.out%d" % i] = a, y
    preds, extra = make_preds(pred_seed, B, fh, fw, T)
    out["pred.seed"] = np.int64(pred_seed)
    out.update(extra)
    wts = torch.from_numpy(LOSS_WEIGHTS)
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        leaves = {k: torch.from_numpy(v).to(dt).requires_grad_(True) for k, v in preds.items()}
        L = head._get_losses(leaves, T)
        assert len(L) == 10
        total = 0
        for i, (k, v) in enumerate(L.items()):
            v = torch.as_tensor(v)
            assert bool(torch.isfinite(v)), (name, k)
            out["loss%s.%s" % (tag, k)] = v.detach().numpy()
            total = total + wts[i].to(dt) * v
        total.backward()
        for k, v in leaves.items():
            g = v.grad
            out["g%s.gnorm.%s" % (tag, k)] = g.double().norm().numpy()
            out["g%s.gsample.%s" % (tag, k)] = g.reshape(-1)[::max(1, g.numel() // 2048)].numpy().copy()
            if k not in HEAT:
                nz = torch.nonzero(g.reshape(-1)).reshape(-1)
                out["g%s.nz.%s" % (tag, k)] = nz.numpy()
                out["g%s.nzval.%s" % (tag, k)] = g.reshape(-1)[nz].numpy().copy()
    print("%-9s B=%d %dx%d: %3d objects, %d exp arguments, losses (fp64) %s" % (
        name, B, h, w, int(lab["mask"].sum()), len(calls),
        " ".join("%.4g" % float(out["loss64." + k]) for k in L)))
    return {name + "." + k: v for k, v in out.items()}, T, preds


def main():
    head = MonoConDenseHeads()
    rboxes = find_radius_boundary_boxes()
    for box, a, b in rboxes:
        print("radius-boundary box %s: reference %d, double %d" % (box.tolist(), a, b))
    hw = []
    for box, a, b in KITTI_BOXES:
        bx = np.array(box, F32)
        bh, bw = (bx[3] - bx[1]) * F32(0.25), (bx[2] - bx[0]) * F32(0.25)
        assert (radius_reference(bh, bw), radius_double(bh, bw)) == (a, b), box
        hw.append((bh, bw, a, b))
    for box, a, b in rboxes:
        hw.append(((box[3] - box[1]) * F32(0.25), (box[2] - box[0]) * F32(0.25), a, b))
    for bh, bw in [(0.5, 0.5), (1.5, 1.5), (3.0, 2.0), (12.0, 30.0), (47.99, 95.99), (160.0, 160.0), (320.0, 320.0), (0.0, 5.0)]:
        hw.append((F32(bh), F32(bw), radius_reference(F32(bh), F32(bw)), radius_double(F32(bh), F32(bw))))
    out = {"radius.hw": np.array([[a, b] for a, b, _, _ in hw], F32),
           "radius.ref": np.array([r for _, _, r, _ in hw], np.int64),
           "radius.double": np.array([r for _, _, _, r in hw], np.int64),
           "radius_boxes_kitti": np.array([b for b, _, _ in KITTI_BOXES], F32),
           "loss_weights": LOSS_WEIGHTS}
    angles, dropped = angle_list()
    out["angles"], out["angles_dropped"] = angles, np.array(dropped, np.float64)

    grp, T, preds = record_group("edge", edge_labels(rboxes, angles), (H, W), SEED + 30, head)
    out.update(grp)
    # what the fixture promises about itself
    assert not T["mask_target"][1].any() and T["mask_target"][0].sum() == 3
    assert int(T["mask_kpt_heatmap_offset"][2].sum()) == 0 and int(T["mask_center2kpt_offset"][2].sum()) > 0
    ind3 = T["indices"][3]
    assert (ind3[:4] == 20 * 96 + 40).all() and (ind3[4:6] == 30 * 96 + 70).all()
    assert T["indices_kpt"][3].reshape(30, 9)[6][:3].tolist() == [0, 25 * 96, 0]
    assert T["mask_kpt_heatmap_offset"][3, 6, :6].tolist() == [1.0] * 6 and int(T["mask_kpt_heatmap_offset"][3, 7:9].sum()) == 0
    for key, tk, ch in (("wh_pred", "wh_target", 0), ("depth_pred", "depth_target", 0), ("dim_pred", "dim_target", 0)):
        sgn = np.sign(preds[key][3, ch, 20, 40] - T[tk][3, :4, ch].numpy())
        assert (sgn > 0).any() and (sgn < 0).any() and max((sgn > 0).sum(), (sgn < 0).sum()) >= 2, (key, sgn)
    assert [int(v) for v in T["alpha_cls_target"][5, :len(angles), 0]] == [
        TargetGenerator()._convert_angle_to_class(torch.tensor(a))[0] for a in angles]

    for name, lab, seed in (("dead", dead_labels(SEED + 21, False), SEED + 31),
                            ("invisible", dead_labels(SEED + 22, True), SEED + 32)):
        grp, T, _ = record_group(name, lab, (H, W), seed, head)
        out.update(grp)
        assert int(T["mask_kpt_heatmap_offset"].sum()) == 0 and float(T["kpt_heatmap_target"].max()) == 0
        assert float(grp[name + ".loss64.loss_kpt_heatmap_offset"]) > 1e12
    assert float(out["invisible.loss64.loss_center2kpt_offset"]) == 0.0 and float(out["dead.loss64.loss_center2kpt_offset"]) > 0
    grp, T, _ = record_group("kitti", kitti_labels(), (384, 1280), SEED + 33, head)
    out.update(grp)
    out["groups"] = np.array(["edge", "dead", "invisible", "kitti"])

    path = os.path.join(HERE, "targets_edge.npz")
    np.savez_compressed(path, **out)
    print("wrote targets_edge.npz: %.1f KB, %d arrays" % (os.path.getsize(path) / 1024, len(out)))


if __name__ == "__main__":
    main()
