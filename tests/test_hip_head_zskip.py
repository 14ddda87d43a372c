"""The heads' backward skips the 64-pixel tiles in which a head's raw gradient is all zero (MONOCON_HIP_HEAD_ZSKIP, default 1;
csrc/kernels_head_train.hip: dpred_pack_kernel writes the tile map, head_bwd_kernel reads it).  A skipped block contributed
exact zeros and everything else is summed in the same order, so every gradient is bit-identical to MONOCON_HIP_HEAD_ZSKIP=0
(torch.equal: -0 == +0, the one admitted difference).  The shapes are the smallest at which the tile logic can go wrong; each
test asserts the partition it relies on from the launcher's own formula (red_rows, kernels_train.hip; head_bwd_args).
The map itself is not read back: the C ABI hands out neither it nor the raw gradient, and no entry point was added for it --
a bit wrongly clear would lose a contribution and fail the comparisons below, a bit wrongly set only costs time.
GPU-only."""
import pytest
import torch

from conftest import GOLDEN_SEED
from hipmonocon import synth

pytestmark = pytest.mark.gpu

TILE = 64                     # dpred_pack_kernel's tile = head_bwd_kernel's staged block (HB_PX)
PRECISIONS = ("fp32", "f16x2")
DX_FUSE = ("0", "1")          # 0: head_bwd_kernel MODE 0 (d stored) + affine pass; 1: MODE 1 + head_dx (MODE 2)


def red_rows(B, rows_per_img):
    r = 256
    while r > 32 and B * ((rows_per_img + r - 1) // r) < 1024:
        r >>= 1
    return r


def partition(B, H, W):
    """(HW, blocks per image, rows per block) of head_bwd_kernel for a B x 3 x H x W batch"""
    HW = (H // 4) * (W // 4)
    bpi = (HW + red_rows(B, HW) - 1) // red_rows(B, HW)
    return HW, bpi, (HW + bpi - 1) // bpi


def to_cuda(batch):
    d = dict(batch)
    d["img"] = batch["img"].cuda()
    d["label"] = {k: v.cuda() for k, v in batch["label"].items()}
    return d


def grads_with(sd, batch, precision, fuse, zskip, monkeypatch, objective=None):
    from model import MonoConDetector
    monkeypatch.setenv("MONOCON_HIP_HEAD_DX_FUSE", fuse)          # both read when the train plan is built
    monkeypatch.setenv("MONOCON_HIP_HEAD_ZSKIP", zskip)
    m = MonoConDetector(34, pretrained_backbone=False)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train().set_precision(precision)
    pred, loss = m(batch)
    (sum(loss.values()) if objective is None else objective(pred, loss)).backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def assert_identical(sd, batch, precision, fuse, monkeypatch, objective=None):
    off = grads_with(sd, batch, precision, fuse, "0", monkeypatch, objective)
    on = grads_with(sd, batch, precision, fuse, "1", monkeypatch, objective)
    assert off.keys() == on.keys() and len(off) > 100
    for n in off:
        assert bool(torch.isfinite(off[n]).all()), n
        assert torch.equal(off[n], on[n]), n
    return off


@pytest.mark.parametrize("fuse", DX_FUSE)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_half_tile_workgroups(golden_sd, precision, fuse, monkeypatch):
    """B = 2, 96x320: 32 rows per workgroup -- half a tile, two workgroups share one word of the map"""
    HW, bpi, rpb = partition(2, 96, 320)
    assert (HW, rpb) == (1920, 32) and TILE % rpb == 0 and HW % TILE == 0
    assert_identical(golden_sd, to_cuda(synth.make_batch(GOLDEN_SEED + 31, 2, 96, 320)), precision, fuse, monkeypatch)


@pytest.mark.parametrize("fuse", DX_FUSE)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_blocks_that_straddle_two_tiles(golden_sd, precision, fuse, monkeypatch):
    """B = 32, 224x288: 126 rows per workgroup, two staged blocks each (64 + 62 pixels), which start at 126 k -- off the tile
    grid, so a block overlaps two tiles and has to test both words"""
    HW, bpi, rpb = partition(32, 224, 288)
    assert (HW, bpi, rpb) == (4032, 32, 126) and rpb % TILE != 0 and rpb > TILE
    assert_identical(golden_sd, to_cuda(synth.make_batch(GOLDEN_SEED + 32, 32, 224, 288)), precision, fuse, monkeypatch)


def place(label, b, slot, col, row, W, H):
    """move object `slot` of image b so that its centre falls on feature pixel (row, col): make_targets_kernel takes the
    centre of gt_bboxes, (x1 + x2) / 2 * (fw / W), truncated"""
    cx, cy = 4.0 * col + 2.0, 4.0 * row + 2.0
    label["gt_bboxes"][b, slot] = torch.tensor([max(cx - 10.0, 0.0), max(cy - 6.0, 0.0), min(cx + 10.0, W - 1.0),
                                                min(cy + 6.0, H - 1.0)])
    x1, y1, x2, y2 = label["gt_bboxes"][b, slot].tolist()
    assert int((x1 + x2) / 2 / 4) == col and int((y1 + y2) / 2 / 4) == row


@pytest.mark.parametrize("fuse", DX_FUSE)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_objects_on_tile_edges_and_images_without_objects(golden_sd, precision, fuse, monkeypatch):
    """B = 3, 96x224 (feature map 24 x 56, 21 tiles): image 0 has exactly two objects, one centred on the FIRST pixel of
    tile 1 (flat 64) and one on the LAST pixel of tile 2 (flat 191); image 1 has a single object; image 2 has none (its mask
    is all zero: every sparse head of it is skipped entirely, its workgroups write zero partials)"""
    H, W = 96, 224
    HW, bpi, rpb = partition(3, H, W)
    assert (HW, rpb) == (1344, 32)
    batch = synth.make_batch(GOLDEN_SEED + 11, 3, H, W)
    lab = batch["label"]
    fw = W // 4
    lab["mask"][0, :2] = 1.0
    for k in ("gt_labels", "gt_labels_3d"):
        lab[k][0, :2] = lab[k][0, 0]
    for k in ("gt_bboxes_3d", "depths", "gt_kpts_2d", "gt_kpts_valid_mask", "centers2d"):
        lab[k][0, 1] = lab[k][0, 0]              # (a valid object's fields, whichever number make_labels drew for image 0)
    place(lab, 0, 0, 64 % fw, 64 // fw, W, H)
    place(lab, 0, 1, 191 % fw, 191 // fw, W, H)
    lab["mask"][0, 2:] = 0.0
    lab["mask"][1, 1:] = 0.0
    lab["mask"][2, :] = 0.0
    assert lab["mask"].sum(1).tolist() == [2.0, 1.0, 0.0]
    g = assert_identical(golden_sd, to_cuda(batch), precision, fuse, monkeypatch)
    # the sparse heads did receive a gradient from those three objects
    assert float(g["head.wh_head.3.weight"].abs().max()) > 0 and float(g["head.depth_head.3.weight"].abs().max()) > 0


USER_SHAPE = (2, 96, 320)


@pytest.mark.parametrize("fuse", DX_FUSE)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ("dense", "one_pixel"))
def test_callers_gradient_of_a_sparse_map(golden_sd, kind, precision, fuse, monkeypatch):
    """the USER pack (mc_backward_pred_grads): the word is formed from loss gradient + caller's gradient.  dense: a random
    gradient for wh_pred sets that head's bit in every tile -- nothing of it may be skipped; one_pixel: non-zero in a single
    pixel that no object touches -- exactly that tile has to be visited.  Either way the term must arrive in the gradients
    as it does with the skip off, and it must arrive at all (compared with the objective without it)."""
    B, H, W = USER_SHAPE
    assert partition(B, H, W)[2] == 32
    batch = to_cuda(synth.make_batch(GOLDEN_SEED + 31, B, H, W))
    G = torch.from_numpy(synth.normalish(GOLDEN_SEED + 33, "zskip.g", (B, 2, H // 4, W // 4))).float().cuda()
    if kind == "one_pixel":
        one = torch.zeros_like(G)
        one[1, 0, 0, 3] = 1.0                    # image 1, tile 0 (feature row 0): make_labels draws no centre above row 16
        G = one
    with_term = assert_identical(golden_sd, batch, precision, fuse, monkeypatch,
                                 lambda pred, loss: sum(loss.values()) + (pred["wh_pred"] * G).sum())
    without = grads_with(golden_sd, batch, precision, fuse, "1", monkeypatch)
    assert not torch.equal(with_term["head.wh_head.3.weight"], without["head.wh_head.3.weight"])


def test_plan_reports_the_switch(golden_sd, monkeypatch, capfd):
    """MONOCON_HIP_PLAN_DEBUG prints what the plan decided: on by default, off with MONOCON_HIP_HEAD_ZSKIP=0"""
    from model import MonoConDetector
    batch = to_cuda(synth.make_batch(GOLDEN_SEED + 31, 2, 64, 128))
    monkeypatch.setenv("MONOCON_HIP_PLAN_DEBUG", "1")
    for zskip, word in ((None, "zero-tile skip on (%d tile words)" % (2 * ((16 * 32 + 63) // 64))), ("0", "zero-tile skip off")):
        monkeypatch.delenv("MONOCON_HIP_HEAD_ZSKIP", raising=False)
        if zskip is not None:
            monkeypatch.setenv("MONOCON_HIP_HEAD_ZSKIP", zskip)
        m = MonoConDetector(34, pretrained_backbone=False)
        m.load_state_dict(golden_sd, strict=True)
        m = m.cuda().train().set_precision("f16x2")
        capfd.readouterr()
        m(batch)
        torch.cuda.synchronize()
        assert word in capfd.readouterr().err, word
