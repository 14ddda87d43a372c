"""Target generation, the ten losses and their gradients on the label shapes training produces and synth.make_labels never
draws, through the Engine methods: masks with holes and poisoned unmasked slots, an empty image inside a batch, objects
whose keypoints are all invisible or off the map, several objects on one pixel, centres in the border pixels with radius 0
and with map-wide splats, boxes whose gaussian radius sits next to an integer, angles outside (-pi, pi] and next to the
bin boundaries (tests/golden/targets_edge.npz, recorded from the reference's own TargetGenerator and _get_losses;
test_oracle_label_edges.py holds the CPU oracle to the same fixture); and the gathered losses at 120 .. 6000 label rows,
where gathered_loss_kernel runs on 2 .. 64 workgroups of 60 .. 94 rows each.  GPU-only.

Which test covers which edge class (all on the groups of the fixture; `edge` image numbers in brackets):
    mask holes + poison [0]            test_targets_vs_reference, test_poisoned_unmasked_slots_change_nothing, *_gradients_*
    empty image inside a batch [1]     test_targets_vs_reference, test_losses_vs_reference
    all keypoints dead [2], dead, invisible   test_targets_vs_reference, test_losses_vs_reference (1e14 and exact 0)
    shared pixels [3]                  test_loss_gradients_vs_autograd_fp64 (non-zero sets), test_shared_pixel_gradients_are_bit_reproducible
    border centres [4]                 test_targets_vs_reference (support and positives of every splat)
    radius-boundary boxes [5], kitti   test_targets_vs_reference, test_train_step_on_edge_labels
    angles [5]                         test_targets_vs_reference (alpha_cls_target / alpha_offset_target bit-equal)
"""
import numpy as np
import pytest
import torch

from conftest import rel_err
from hipmonocon import netspec, synth
from label_edge_fixture import GROUPS, HEAT, LO, HI, Group, raw_leaves, weighted_total
from test_hip_train_step import PRECISIONS, LOSS_TOL, build, oracle_losses_fp64, to_cuda

pytestmark = pytest.mark.gpu

PRED_KEYS = tuple(k for k, _ in netspec.PRED_KEYS)
REGRESSION = tuple(k for k in PRED_KEYS if k not in HEAT)
EXACT = ("indices", "indices_kpt", "mask_target", "mask_center2kpt_offset", "mask_kpt_heatmap_offset", "alpha_cls_target",
         "wh_target", "offset_target", "dim_target", "depth_target", "center2kpt_offset_target", "kpt_heatmap_offset_target",
         "alpha_offset_target")


@pytest.fixture(scope="module")
def eng():
    from hipmonocon.engine import Engine
    return Engine()


def cuda(d):
    return {k: v.cuda().contiguous() for k, v in d.items()}


def assert_targets_equal_reference(T, ref, tag):
    assert set(T) == set(EXACT) | {"center_heatmap_target", "kpt_heatmap_target"}
    for name in EXACT:                                                       # integers, masks and the fp32 op sequence: exact
        got = T[name].cpu().numpy()
        assert got.shape == ref(name).shape and np.array_equal(got, ref(name)), (tag, name)
    for name in ("center_heatmap_target", "kpt_heatmap_target"):
        got, want = T[name].cpu().numpy(), ref(name)
        assert np.array_equal(got == 1.0, want == 1.0), (tag, name)           # which pixels are positives
        assert np.array_equal(got > 0, want > 0), (tag, name)                 # support of every splat
        err = float(np.abs(got - want).max())
        print("%s %s: max |target - reference| = %.2e (bound 2e-7)" % (tag, name, err))
        assert err < 2e-7, (tag, name)                                        # expf vs torch.exp: <= 1 ulp


@pytest.mark.parametrize("group", GROUPS)
def test_targets_vs_reference(eng, group):
    """make_targets_kernel on every group of the fixture: integer and mask tensors and the fp32 regression targets bit-equal
    to the reference's, heat-map positives and support equal, values within 2e-7 (measured: 6.0e-8).
    The groups `edge` and `kitti` hold boxes whose radius sits next to an integer: with `a * b - c` contracted into one fma
    in gaussian_radius_ref the kernel splatted a radius one smaller on three of the seven (the support test below failed,
    and loss_center_heatmap was 2.4e-4 / 1.9e-4 off in test_losses_vs_reference)"""
    G = Group(group)
    T = eng.make_targets(cuda(G.labels()), (G.H, G.W), (G.fh, G.fw))
    assert_targets_equal_reference(T, lambda k: G[k], group)


def test_poisoned_unmasked_slots_change_nothing(eng):
    """NaN boxes / angles / keypoints, class 7 and stale finite values in slots whose mask is 0: the same 15 tensors, bit for
    bit, as with those slots zeroed -- and nothing of them is NaN"""
    G = Group("edge")
    lab = G.labels()
    assert bool(torch.isnan(lab["gt_bboxes"]).any()) and float(lab["gt_labels"].max()) == 7
    clean = {k: v.clone() for k, v in lab.items()}
    for k, v in clean.items():
        if k != "mask":
            v[lab["mask"] == 0] = 0
    assert not any(bool(torch.isnan(v).any()) for v in clean.values())
    T = eng.make_targets(cuda(lab), (G.H, G.W), (G.fh, G.fw))
    Tc = eng.make_targets(cuda(clean), (G.H, G.W), (G.fh, G.fw))
    for k in T:
        assert torch.equal(T[k], Tc[k]), k
        assert not bool(torch.isnan(T[k].float()).any()), k


def loss_bound(ref):
    return 1e-4 * abs(ref) + 1e-6


@pytest.mark.parametrize("group", GROUPS)
def test_losses_vs_reference(eng, group):
    """each of the ten losses within 1e-4 |ref| + 1e-6 of the reference's float64 value, on the kernel's own targets:
    including loss_kpt_heatmap_offset ~ 1e14 of the groups without a live keypoint (the focal loss's num_pos == 0 branch,
    an unmasked numerator over 0 + 1e-12) and the exact 0 of loss_center2kpt_offset in `invisible`.
    measured, worst |loss - ref| / |ref| over the four groups: center_heatmap 8.6e-8, wh 3.1e-8, offset 1.3e-8, dim 2.8e-8,
    center2kpt_offset 3.2e-8, kpt_heatmap 4.8e-8, kpt_heatmap_offset 4.9e-8, alpha_cls 1.5e-7, alpha_reg 4.2e-8, depth 6.8e-8"""
    G = Group(group)
    T = eng.make_targets(cuda(G.labels()), (G.H, G.W), (G.fh, G.fw))
    L = eng.losses(cuda(G.preds()), T).cpu()
    assert bool(torch.isfinite(L).all())
    for i, k in enumerate(netspec.LOSS_KEYS):
        ref = float(G["loss64." + k])
        print("%s %s: %.9g vs %.9g, rel %.2e" % (group, k, float(L[i]), ref, abs(float(L[i]) - ref) / max(abs(ref), 1e-30)))
    for i, k in enumerate(netspec.LOSS_KEYS):
        ref = float(G["loss64." + k])
        assert abs(float(L[i]) - ref) <= loss_bound(ref), (group, k, float(L[i]), ref)
    if group in ("dead", "invisible"):
        assert float(G["loss64.loss_kpt_heatmap_offset"]) > 1e13
    if group == "invisible":
        assert float(G["loss64.loss_center2kpt_offset"]) == 0.0 and float(L[4]) == 0.0


def autograd_fp64(preds, T, w, wrt_pred, max_objs=30):
    """float64 autograd through the oracle's losses: gradients wrt the maps themselves, or wrt the raw 1x1 outputs"""
    from oracle import monocon_oracle as O
    if wrt_pred:
        leaves = {k: v.double().requires_grad_(True) for k, v in preds.items()}
        act = leaves
    else:
        leaves, act = raw_leaves(preds)
    weighted_total(O.losses(act, T, max_objs=max_objs), w).backward()
    return {k: v.grad for k, v in leaves.items()}


def check_gradients(d, ref, preds, tag, wrt_pred, nz_ref=None):
    """rel_err < 2e-4 per map; on the regression maps the same set of non-zero pixels; on-clamp heat-map entries exactly 0
    (raw variant) / the reference's value (pred variant)"""
    for k in PRED_KEYS:
        got = d[k].cpu()
        assert bool(torch.isfinite(got).all()), (tag, k)
        e = rel_err(got, ref[k])
        print("%s %s %s: rel_err %.2e (bound 2e-4)" % (tag, "pred" if wrt_pred else "raw", k, e))
    for k in PRED_KEYS:
        got = d[k].cpu()
        assert rel_err(got, ref[k]) < 2e-4, (tag, k, rel_err(got, ref[k]))
        if k in REGRESSION:
            nz = torch.nonzero(got.reshape(-1)).reshape(-1)
            assert torch.equal(nz, torch.nonzero(ref[k].reshape(-1)).reshape(-1)), (tag, k)
            if nz_ref is not None:
                assert np.array_equal(nz.numpy(), nz_ref(k)), (tag, k)              # ... which is the reference's own set
        else:
            on = (preds[k] == LO) | (preds[k] == HI)
            assert int(on.sum()) >= 48
            if wrt_pred:
                assert rel_err(got[on], ref[k][on]) < 2e-4 and float(ref[k][on].abs().min()) > 0, (tag, k)
            else:
                assert float(got[on].abs().max()) == 0.0 and float(ref[k][on].abs().max()) == 0.0, (tag, k)


@pytest.mark.parametrize("wrt_pred", [False, True], ids=["raw", "pred"])
@pytest.mark.parametrize("group", GROUPS)
def test_loss_gradients_vs_autograd_fp64(eng, group, wrt_pred):
    """losses_backward on every group against float64 autograd through O.losses, unequal loss weights.
    measured, worst rel_err over the four groups and both variants (bound 2e-4): center_heatmap 2.6e-7, kpt_heatmap 2.4e-7,
    wh 4.5e-8, offset 3.0e-8, kpt_heatmap_offset 4.4e-7, center2kpt_offset 3.5e-8, dim 1.0e-7, depth 1.1e-7, alpha_cls 1.0e-7,
    alpha_offset 3.0e-8"""
    G = Group(group)
    preds, w = G.preds(), G.weights()
    T = eng.make_targets(cuda(G.labels()), (G.H, G.W), (G.fh, G.fw))
    ref = autograd_fp64(preds, {k: v.cpu() for k, v in T.items()}, w, wrt_pred)
    d = eng.losses_backward(cuda(preds), T, w.cuda(), wrt_pred=wrt_pred)
    check_gradients(d, ref, preds, group, wrt_pred, nz_ref=(lambda k: G["g64.nz." + k]) if wrt_pred else None)
    if wrt_pred:                # the reference's own values on its non-zero entries
        for k in REGRESSION:
            nz = torch.from_numpy(G["g64.nz." + k])
            if len(nz):
                assert rel_err(d[k].cpu().reshape(-1)[nz], G["g64.nzval." + k]) < 2e-4, (group, k)


@pytest.mark.parametrize("wrt_pred", [False, True], ids=["raw", "pred"])
def test_shared_pixel_gradients_are_bit_reproducible(eng, wrt_pred):
    """the group with four objects of one class on one pixel, two of different classes on another and dead + live keypoint
    gathers meeting on pixel 0: two runs of the atomic scatter give bit-equal maps (measured: they do, in both variants)"""
    G = Group("edge")
    preds, w = cuda(G.preds()), G.weights().cuda()
    T = eng.make_targets(cuda(G.labels()), (G.H, G.W), (G.fh, G.fw))
    assert int((T["indices"][3, :4] == T["indices"][3, 0]).sum()) == 4
    runs = []
    for _ in range(2):
        d = eng.losses_backward(preds, T, w, wrt_pred=wrt_pred)
        torch.cuda.synchronize()
        runs.append({k: v.clone() for k, v in d.items()})
    for k in PRED_KEYS:
        assert torch.equal(runs[0][k], runs[1][k]), k


def fast_preds(seed, B, fh, fw):
    """prediction maps for the many-row cases from a seeded CPU generator (make_decode_inputs' ranges; its hash stream takes
    minutes at B = 241): heat-maps in [1e-4, 1 - 1e-4] with entries on both clamp values, positive dimensions"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda c, m=0.0, s=1.0: torch.randn((B, c, fh, fw), generator=gen) * s + m              # noqa: E731
    un = lambda c, lo, hi: torch.rand((B, c, fh, fw), generator=gen) * (hi - lo) + lo               # noqa: E731
    d = {"center_heatmap_pred": un(3, -0.01, 1.01).clamp(1e-4, 1 - 1e-4), "kpt_heatmap_pred": un(9, -0.01, 1.01).clamp(1e-4, 1 - 1e-4),
         "wh_pred": rn(2, 12.0, 4.0), "offset_pred": un(2, 0.0, 1.0), "kpt_heatmap_offset_pred": rn(2),
         "center2kpt_offset_pred": rn(18, 0.0, 3.0), "dim_pred": rn(3).abs() + 1.0,
         "depth_pred": torch.cat([un(1, 2.0, 60.0), un(1, -1.0, 3.0)], 1), "alpha_cls_pred": rn(12), "alpha_offset_pred": rn(12, 0.0, 0.3)}
    for k in HEAT:
        assert int((d[k] == LO).sum()) >= 24 and int((d[k] == HI).sum()) >= 24
    return {k: d[k].contiguous() for k in PRED_KEYS}


@pytest.mark.parametrize("B,max_objs", [(4, 30), (32, 30), (91, 45), (128, 32), (241, 17), (200, 30)],
                         ids=lambda v: str(v))
def test_many_label_rows_vs_oracle_fp64(eng, B, max_objs):
    """B * max_objs = 120 (two workgroups of gathered_loss_kernel), 960 (the benchmark's fifteen), 4095 / 4096 / 4097 (the
    switch from 64 rows per workgroup to the 64-workgroup cap: 64 x 64, 64 x 64, 64 x 65 rows) and 6000 (64 x 94), labels
    from synth.make_labels at 192x384 with up to max_objs objects per image: targets equal to O.make_targets, losses within
    1e-4 |ref| + 1e-6 and both gradient variants within 2e-4 of the oracle in float64, regression non-zero sets equal.
    measured, worst over the six shapes: losses 5.9e-8 relative (dim), gradient maps 1.2e-6 (kpt_heatmap_offset), 3.4e-7 on
    the heat-maps, <= 2.0e-7 on the other regression maps"""
    from oracle import monocon_oracle as O
    H, W = 192, 384
    fh, fw = H // 4, W // 4
    assert B * max_objs in (120, 960, 4095, 4096, 4097, 6000)
    lab = synth.make_labels(1000 + B, B, H, W, max_objs=max_objs, min_objs=1, max_gen=max_objs)
    assert int(lab["mask"].sum()) >= B and float(lab["mask"].sum(1).min()) >= 1
    lab = {k: torch.from_numpy(v) for k, v in lab.items()}
    Tref = O.make_targets(lab, (H, W), (B, 64, fh, fw), max_objs=max_objs)
    T = eng.make_targets(cuda(lab), (H, W), (fh, fw), max_objs=max_objs)
    for k, v in Tref.items():
        got = T[k].cpu()
        if v.dtype in (torch.long, torch.bool):
            assert torch.equal(got, v), k
        else:
            assert float((got - v).abs().max()) < 2e-7, k
    preds = fast_preds(B, B, fh, fw)
    dev = cuda(preds)
    with torch.no_grad():
        L64 = O.losses({k: v.double() for k, v in preds.items()}, Tref, max_objs=max_objs)
    L = eng.losses(dev, T, max_objs=max_objs).cpu()
    assert bool(torch.isfinite(L).all())
    for i, k in enumerate(netspec.LOSS_KEYS):
        ref = float(L64[k])
        print("rows %d %s: %.9g vs %.9g, rel %.2e" % (B * max_objs, k, float(L[i]), ref, abs(float(L[i]) - ref) / abs(ref)))
        assert abs(float(L[i]) - ref) <= loss_bound(ref), (k, float(L[i]), ref)
    w = torch.tensor([1.0, 0.5, 2.0, 1.5, 1.0, 0.7, 1.0, 3.0, 1.0, 0.25])
    Tcpu = {k: v.cpu() for k, v in T.items()}
    for wrt_pred in (False, True):
        ref = autograd_fp64(preds, Tcpu, w, wrt_pred, max_objs)
        d = eng.losses_backward(dev, T, w.cuda(), max_objs=max_objs, wrt_pred=wrt_pred)
        check_gradients(d, ref, preds, "rows %d" % (B * max_objs), wrt_pred)
        del ref, d


# ------------------------------------------------------------------------------------------------ whole train step
def edge_batch():
    """synth.make_conditioned_batch at the shape of the conditioned fixture 0 (B = 4, 64x64), labels edited: image 0 a mask
    with a hole and poison in it, image 1 empty, image 2 two objects on one pixel, image 3 a radius-boundary box"""
    from conftest import load_golden
    from oracle import monocon_oracle as O
    g = load_golden("train_cond_0.npz")
    B, H, W = (int(x) for x in g["shape"])
    batch = synth.make_conditioned_batch(int(g["seed"]), B, H, W)
    lab = batch["label"]
    src = int(lab["mask"][0].sum()) - 1                       # a valid slot of image 0 to copy complete objects from
    for b in range(B):
        for s in range(4):
            for v in lab.values():
                v[b, s] = v[0, src].clone()
    lab["mask"][:] = 0
    lab["mask"][0, [0, 2]] = 1
    for k, v in lab.items():
        if k != "mask":
            v[0, 1] = float("nan")
    lab["gt_labels"][0, 1] = 7
    lab["gt_bboxes"][0, 3] = torch.tensor([1e6, 1e6, 2e6, 2e6])            # stale, far outside, behind the last valid slot
    lab["gt_bboxes"][0, 0] = torch.tensor([2.0, 3.0, 30.0, 40.0])
    lab["gt_bboxes"][0, 2] = torch.tensor([20.0, 10.0, 63.0, 60.0])
    lab["mask"][2, :2] = 1
    lab["gt_bboxes"][2, 0] = torch.tensor([20.0, 22.0, 46.0, 44.0])        # centre (33, 33) -> pixel (8, 8)
    lab["gt_bboxes"][2, 1] = torch.tensor([5.5, 2.0, 63.0, 69.0])          # centre (34.25, 35.5) -> pixel (8, 8)
    lab["depths"][2, 1] = lab["depths"][2, 0] * 2
    e = load_golden("targets_edge.npz")
    fit = [(h, w, r, d) for (h, w), r, d in zip(e["radius.hw"], e["radius.ref"], e["radius.double"])
           if r != d and 2 * h < H and 2 * w < W]
    bh, bw, r, dbl = fit[0]
    box = torch.tensor([0.0, 0.0, 4 * bw, 4 * bh])                           # (x2 - 0) * 0.25 == bw exactly
    assert float((box[2] - box[0]) * 0.25) == bw and float((box[3] - box[1]) * 0.25) == bh
    assert max(0, int(O.gaussian_radius((box[3] - box[1]) * 0.25, (box[2] - box[0]) * 0.25))) == r != dbl
    lab["mask"][3, 0] = 1
    lab["gt_bboxes"][3, 0] = box
    return batch, (H, W)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_train_step_on_edge_labels(cond_sd, precision):
    """model(batch) + backward() on a conditioned batch whose labels hold a mask hole with poisoned slots, an empty image, a
    shared pixel and a radius-boundary box: losses within LOSS_TOL of the float64 oracle, gradients finite and of the
    oracle's total norm (5 %; measured: 1673.39 vs 1673.38 in all three precisions), and neither label check trips over the
    poisoned unmasked slots"""
    from hipmonocon.train import labels_ok_on_host
    from oracle import monocon_oracle as O
    batch, (H, W) = edge_batch()
    assert labels_ok_on_host(batch["label"], (H, W))
    live = {k: (v.clone().requires_grad_(True) if v.dtype == torch.float32 and "running" not in k else v.clone())
            for k, v in cond_sd.items()}
    _, T, L, _ = O.train_forward(live, batch)
    assert T["mask_target"].sum(1).tolist() == [2, 0, 2, 1] and int(T["indices"][2, 0]) == int(T["indices"][2, 1]) == 8 * 16 + 8
    sum(L.values()).backward()
    ref_norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in live.values()
                                    if getattr(p, "grad", None) is not None)))
    L64 = oracle_losses_fp64(cond_sd, batch)
    m = build(cond_sd, precision)
    _, loss = m(to_cuda(batch))
    sum(loss.values()).backward()
    torch.cuda.synchronize()
    for k, v in loss.items():
        print("%s %s: %.9g vs %.9g" % (precision, k, float(v.detach()), L64[k]))
        assert abs(float(v.detach()) - L64[k]) <= LOSS_TOL * abs(L64[k]) + 1e-7, (k, float(v.detach()), L64[k])
    g = torch.cat([p.grad.flatten() for p in m.parameters() if p.grad is not None])
    assert bool(torch.isfinite(g).all())
    print("%s: gradient norm %.6g vs %.6g" % (precision, float(g.double().norm()), ref_norm))
    assert abs(float(g.double().norm()) - ref_norm) <= 0.05 * ref_norm, (float(g.double().norm()), ref_norm)


def test_masked_slot_outside_the_map_still_raises(cond_sd):
    """one MASKED slot whose centre is outside the map: IndexError before anything is launched, as in the reference (whose
    heat-map index is out of bounds); the host-side check sends such a batch to the device-side one"""
    from hipmonocon.train import labels_ok_on_host
    batch, (H, W) = edge_batch()
    batch["label"]["gt_bboxes"][2, 1] = torch.tensor([W + 8.0, 10.0, W + 40.0, 30.0])
    assert not labels_ok_on_host(batch["label"], (H, W))
    m = build(cond_sd, "fp32")
    with pytest.raises(IndexError):
        m(to_cuda(batch))
