"""Pin the CPU oracle's target generation and losses to the reference on the label shapes training produces and
synth.make_labels never draws (tests/golden/targets_edge.npz, recorded from the reference's own TargetGenerator and
MonoConDenseHeads._get_losses by tests/golden/make_targets_edge_golden.py): masks with holes and poisoned unmasked slots,
an empty image inside a batch, objects whose keypoints are all invisible or off the map, several objects on one pixel,
centres in the border pixels, boxes whose gaussian radius sits next to an integer, angles outside (-pi, pi] and next to
the bin boundaries.  CPU-only."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, gsample
from label_edge_fixture import GROUPS, HEAT, Group, golden_exp, weighted_total
from oracle import monocon_oracle as O


def test_gaussian_radius_vs_reference():
    """O.gaussian_radius against the (h, w, radius) triples the reference's own gaussian_radius returned on 0-dim fp32
    tensors.  The first seven are boxes on which a double evaluation of the same formula floors to another integer -- the
    three 384x1280 boxes below (7 / 5 / 11, a double evaluation gives 6 / 4 / 10) and four found by the generator's seeded
    search at 192x384.  An oracle that converts its arguments with float() and computes in double fails here on all
    seven."""
    g = load_golden("targets_edge.npz")
    hw, ref, dbl = g["radius.hw"], g["radius.ref"], g["radius.double"]
    assert hw.dtype == np.float32 and len(hw) >= 12
    disagree = np.nonzero(ref != dbl)[0]
    assert len(disagree) >= 6 and disagree.tolist() == list(range(len(disagree)))
    # the three boxes of the report are the fixture's first three, at the radii the reference gives them
    boxes = g["radius_boxes_kitti"]
    assert np.array_equal(boxes, np.array([[251.7559356689453, 231.15426635742188, 358.4798583984375, 383.0],
                                           [1125.3323974609375, 29.458070755004883, 1252.580810546875, 100.57401275634766],
                                           [584.727783203125, 218.52171325683594, 832.7520141601562, 383.0]], np.float32))
    assert np.array_equal(hw[:3, 0], (boxes[:, 3] - boxes[:, 1]) * np.float32(0.25))
    assert np.array_equal(hw[:3, 1], (boxes[:, 2] - boxes[:, 0]) * np.float32(0.25))
    assert ref[:3].tolist() == [7, 5, 11] and dbl[:3].tolist() == [6, 4, 10]
    for (h, w), r in zip(hw, ref):
        assert max(0, int(O.gaussian_radius(torch.tensor(h), torch.tensor(w)))) == r, (h, w, r)
        assert max(0, int(O.gaussian_radius(h, w))) == r, (h, w, r)          # numpy fp32 scalars: the same arithmetic


@pytest.mark.parametrize("group", GROUPS)
def test_targets_exact(monkeypatch, group):
    """O.make_targets on the fixture's labels: all 15 tensors bit-equal to the reference, with the reference host's fp32 exp
    results substituted as in test_oracle_golden.test_targets_exact.  The groups `edge` and `kitti` fail on an oracle whose
    gaussian_radius computes in double: e.g. on the `kitti` box [251.7559356689453, 231.15426635742188, 358.4798583984375,
    383.0] such an oracle splats radius 6 where the reference splats radius 7 (center_heatmap_target and every
    kpt_heatmap_target plane of that object differ; its exp argument of shape (13, 13) is one the reference never took)."""
    G = Group(group)
    used = golden_exp(monkeypatch, G.exp_table())
    T = O.make_targets(G.labels(), (G.H, G.W), (G.B, 64, G.fh, G.fw))
    monkeypatch.undo()
    assert used == set(range(int(G["exp.n"])))
    assert len(T) == 15
    for k, v in T.items():
        ref = G[k]
        assert tuple(v.shape) == ref.shape and v.numpy().dtype == ref.dtype, k
        assert np.array_equal(v.numpy(), ref), k              # same fp32 op sequence -> bit equal (no NaN in any target)
        assert not np.isnan(ref.astype(np.float64)).any(), k


def test_fixture_holds_what_it_promises():
    """the edge classes are in the fixture (read from its targets, not from the generator's word)"""
    G = Group("edge")
    lab, T = G.labels(), G.targets()
    m = lab["mask"]
    assert m[0].nonzero().flatten().tolist() == [0, 2, 5] and bool(torch.isnan(lab["gt_bboxes"][0, [1, 3, 4]]).all())
    assert lab["gt_labels"][0, [1, 3, 4]].tolist() == [7.0] * 3 and bool(torch.isfinite(lab["gt_bboxes"][0, 6:]).all())
    assert T["mask_target"][0].nonzero().flatten().tolist() == [0, 1, 2]                    # compacted
    assert float(m[1].sum()) == 0 and float(m[0].sum()) > 0 and float(m[2].sum()) > 0       # empty image between two others
    assert float(T["mask_kpt_heatmap_offset"][2].sum()) == 0 and float(T["kpt_heatmap_target"][2].max()) == 0
    assert float(T["mask_center2kpt_offset"][2].sum()) > 0                                  # visible, but off the map
    ind = T["indices"][3]
    assert ind[:4].tolist() == [20 * G.fw + 40] * 4 and T["wh_target"][3, :4, 0].unique().numel() == 4
    assert ind[4:6].tolist() == [30 * G.fw + 70] * 2 and lab["gt_labels"][3, 4:6].tolist() == [1.0, 2.0]
    ik = T["indices_kpt"][3].reshape(30, 9)
    assert ik[6, 0] == 0 and float(T["mask_kpt_heatmap_offset"][3, 6, 0]) == 1              # live gather of pixel 0 ...
    assert float(lab["gt_kpts_2d"][3, 6, 0]) * 0.25 == -0.5                                 # ... from a coordinate in (-1, 0)
    assert ik[7].tolist() == [0] * 9 and float(T["mask_kpt_heatmap_offset"][3, 7].sum()) == 0        # ... beside dead ones
    n4 = int(m[4].sum())
    xs, ys = (T["indices"][4, :n4] % G.fw).tolist(), (T["indices"][4, :n4] // G.fw).tolist()
    for corner in ((0, 0), (G.fw - 1, 0), (0, G.fh - 1), (G.fw - 1, G.fh - 1)):
        assert list(zip(xs, ys)).count(corner) >= 2, corner
    assert 0 in ys and G.fh - 1 in ys and 0 in xs and G.fw - 1 in xs
    assert float(lab["gt_bboxes"][4, n4 - 1, 2]) == np.float32(G.W - 0.01)
    hm = T["center_heatmap_target"][4]
    assert int((hm == 1).sum()) >= 8 and float((hm > 0).float().mean()) > 0.9              # radius 0 peaks and map-wide splats
    ang = G.g["angles"]
    assert len(ang) >= 20 and len(G.g["angles_dropped"]) == 0
    for v in (0.0, np.pi, -np.pi, 2 * np.pi, -2 * np.pi, 2 * np.pi + 0.3, 4 * np.pi):
        assert np.float32(v) in ang
    assert np.signbit(ang[1]) and ang[1] == 0
    assert np.array_equal(lab["gt_bboxes_3d"][5, :len(ang), 6].numpy(), ang)
    cls = T["alpha_cls_target"][5, :len(ang), 0]
    assert float(cls.min()) >= 0 and float(cls.max()) <= 11
    nb = 0
    for k in (1, 6, 12, -3):                # fp32 neighbours (-3 .. +1 ulp) of a bin boundary land in two different bins
        f = np.float32(k * np.pi / 6 - np.pi / 12)
        i = int(np.nonzero(ang == f)[0][0])
        assert ang[i - 1] == np.nextafter(f, np.float32(-np.inf)) and ang[i + 1] == np.nextafter(f, np.float32(np.inf))
        assert bool((np.diff(ang[i - 3:i + 2]) > 0).all())
        nb += len({float(c) for c in cls[i - 3:i + 2]}) == 2
    assert nb == 4
    for name in ("dead", "invisible"):
        D = Group(name)
        assert float(D["mask_kpt_heatmap_offset"].sum()) == 0 and float(D["kpt_heatmap_target"].max()) == 0
        assert float(D["loss64.loss_kpt_heatmap_offset"]) > 1e13
    assert float(Group("invisible")["loss64.loss_center2kpt_offset"]) == 0.0
    assert float(Group("dead")["mask_center2kpt_offset"].sum()) > 0


@pytest.mark.parametrize("group", GROUPS)
def test_losses_fp64(group):
    """O.losses on float64 maps and the reference's targets against the reference's float64 losses (1e-9 relative: the same
    operations, summed in another order at most; the exact 0 of an all-invisible batch stays an exact 0).  The reference's
    loss_alpha_cls comes out as an fp32 tensor whatever the maps' type (its cross-entropy calls label.float()): that one is
    held to 1e-6, a mean of fp32 terms that each carry a 6e-8 rounding."""
    G = Group(group)
    L = O.losses({k: v.double() for k, v in G.preds().items()}, G.targets())
    assert tuple(L) == O.LOSS_ORDER
    for k, v in L.items():
        ref = float(G["loss64." + k])
        assert np.isfinite(ref)
        assert (G["loss64." + k].dtype == np.float32) == (k == "loss_alpha_cls"), k
        assert abs(float(v) - ref) <= (1e-6 if k == "loss_alpha_cls" else 1e-9) * abs(ref), (k, float(v), ref)


@pytest.mark.parametrize("group", GROUPS)
def test_losses_fp32(group):
    """the same in float32, at the tolerance test_train_step_losses_and_grads holds the losses to (2e-5 relative)"""
    G = Group(group)
    L = O.losses(G.preds(), G.targets())
    for k, v in L.items():
        ref = float(G["loss32." + k])
        assert abs(float(v) - ref) <= 2e-5 * abs(ref), (k, float(v), ref)
        assert abs(ref - float(G["loss64." + k])) <= 1e-4 * abs(float(G["loss64." + k])), k       # (the reference's own fp32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("group", GROUPS)
def test_loss_gradients_vs_reference_autograd(group, dtype):
    """autograd through O.losses of sum_i w_i loss_i (unequal w) with respect to every prediction map against the
    reference's autograd through _get_losses: norm within 2e-3, strided sample within 5e-3 (the bounds of
    test_train_step_losses_and_grads), and on the eight regression maps the same set of non-zero entries with the same
    values -- a gather of a wrong pixel or a masked-out slot leaking through changes the set."""
    G = Group(group)
    tag = "g32" if dtype == torch.float32 else "g64"
    leaves = {k: v.to(dtype).requires_grad_(True) for k, v in G.preds().items()}
    weighted_total(O.losses(leaves, G.targets()), G.weights()).backward()
    for k, v in leaves.items():
        gn = float(G["%s.gnorm.%s" % (tag, k)])
        assert abs(float(v.grad.double().norm()) - gn) <= 2e-3 * gn + 1e-7, k
        assert rel_err(gsample(v.grad), G["%s.gsample.%s" % (tag, k)]) < 5e-3, k
        if k in HEAT:
            continue
        nz = torch.nonzero(v.grad.reshape(-1)).reshape(-1)
        assert np.array_equal(nz.numpy(), G["%s.nz.%s" % (tag, k)]), k
        if len(nz):          # (an all-invisible batch leaves the centre-to-keypoint map without any gradient)
            assert rel_err(v.grad.reshape(-1)[nz], G["%s.nzval.%s" % (tag, k)]) < 5e-3, k
