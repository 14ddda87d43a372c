"""mc_nms3d (greedy 3D-box NMS of the decode's boxes on the device), Engine.nms3d / decode(nms=) and the detector with the
three test_config keys.  GPU-only.  keep_out and suppressed_by are compared EXACTLY with the CPU reference of
tests/nms_reference.py, whose overlaps are the oracle's; every threshold keeps the oracle overlaps of the participating,
class-compatible pairs at least EXACT_MARGIN away (the module's docstring gives the reasoning), which each test asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import nms_reference as NR
from test_hip_kitti_format import _assert_vis_equal, assert_annos_close

pytestmark = pytest.mark.gpu

MODES = ("bev", "3d")


@pytest.fixture(scope="module")
def eng():
    from hipmonocon.engine import Engine
    return Engine()


def device_nms(eng, box2d, box3d, cls, keep_in, mode, thr, class_agnostic):
    """(B,K,..) host arrays -> keep_nms (B,K) uint8, suppressed_by (B,K) int32 of one mc_nms3d launch"""
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(eng.device)
    R = {"box2d": up(box2d, np.float32), "box3d": up(box3d, np.float32), "cls": up(cls, np.int64), "keep_thr": up(keep_in, np.uint8)}
    out = eng.nms3d(R, thr, mode=MODES[mode], class_agnostic=class_agnostic)
    assert out["keep_nms"].dtype == torch.uint8 and out["suppressed_by"].dtype == torch.int32
    return out["keep_nms"].cpu().numpy(), out["suppressed_by"].cpu().numpy()


def assert_same(got, want, tag):
    (gk, gb), (wk, wb) = got, want
    assert np.array_equal(gk, wk), (tag, "keep", np.argwhere(gk != wk)[:8].tolist())
    assert np.array_equal(gb, wb), (tag, "suppressed_by", np.argwhere(gb != wb)[:8].tolist())


def single(box3d, scores, cls=None, keep_in=None):
    """one image from rows of box3d and scores -> the (1,K,..) arrays"""
    K = len(box3d)
    box2d = np.zeros((1, K, 5), dtype=np.float32)
    box2d[0, :, 4] = scores
    cls = np.zeros((1, K), np.int64) if cls is None else np.asarray(cls, np.int64)[None]
    keep_in = np.ones((1, K), np.uint8) if keep_in is None else np.asarray(keep_in, np.uint8)[None]
    return box2d, np.asarray(box3d, np.float32)[None], cls, keep_in


def check_single(eng, box3d, scores, mode, thr, cls=None, keep_in=None, class_agnostic=False, tag=""):
    """one image on the device against the reference; returns the (keep, suppressed_by) lists"""
    a = single(box3d, scores, cls, keep_in)
    want = NR.nms_reference(a[0][0], a[1][0], a[2][0], a[3][0], mode, thr, class_agnostic)
    gk, gb = device_nms(eng, *a, mode, thr, class_agnostic)
    assert_same((gk[0], gb[0]), want[:2], tag)
    return gk[0].tolist(), gb[0].tolist()


# ------------------------------------------------------------------------------------------------ 1. closed forms
@pytest.mark.parametrize("mode", [0, 1])
def test_closed_forms(eng, mode):
    """A, B, C at x = 0, 1, 2: IoU(A,B) = IoU(B,C) = 0.6, IoU(A,C) = 1/3, threshold 0.5"""
    b = NR.closed_form_boxes()
    # A > B > C: A and C are kept, B is A's -- a dead B must not kill C
    assert check_single(eng, b[:3], [0.9, 0.8, 0.7], mode, 0.5) == ([1, 0, 1], [-1, 0, -1])
    # B > A > C: only B is kept
    assert check_single(eng, b[:3], [0.8, 0.9, 0.7], mode, 0.5) == ([0, 1, 0], [1, -1, 1])
    # D: C's footprint with no height in common -- dies in mode 0, survives in mode 1
    got = check_single(eng, b, [0.9, 0.8, 0.7, 0.6], mode, 0.5)
    assert got == (([1, 0, 1, 0], [-1, 0, -1, 2]) if mode == 0 else ([1, 0, 1, 1], [-1, 0, -1, -1]))
    # classes
    assert check_single(eng, b[:3], [0.9, 0.8, 0.7], mode, 0.5, cls=[0, 1, 0]) == ([1, 1, 1], [-1, -1, -1])
    assert check_single(eng, b[:3], [0.9, 0.8, 0.7], mode, 0.5, cls=[0, 1, 0], class_agnostic=True) == ([1, 0, 1], [-1, 0, -1])
    # the ends of the threshold's range: at 0 every overlapping pair suppresses, at 1 none
    assert check_single(eng, b[:3], [0.9, 0.8, 0.7], mode, 0.0)[0] == [1, 0, 0]
    assert check_single(eng, b[:3], [0.9, 0.8, 0.7], mode, 1.0)[0] == [1, 1, 1]


# ------------------------------------------------------------------------------------------------ 2. clustered random boxes
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 100])
def test_clustered_random_boxes(eng, K):
    """B = 3 images with their own seeds, ~80 % participants, classes 0..2; nominal thresholds 0.1 / 0.3 / 0.5 moved to the
    centre of the widest gap of the oracle's overlaps, both modes, class-aware and class-agnostic.  63, 64 and 65: the word
    and wave boundaries of the bit matrix and the ballots."""
    B, ran = 3, 0
    for mode in (0, 1):
        cases = [NR.clustered_case(1000 * K + b, K, mode) for b in range(B)]
        box2d, box3d, cls, keep_in = (np.stack([c[i] for c in cases]) for i in range(4))
        for class_agnostic in (False, True):
            oks = [NR.compatible(c[2], c[4], class_agnostic) for c in cases]
            values = np.concatenate([c[5][ok] for c, ok in zip(cases, oks)])
            for nominal in (0.1, 0.3, 0.5):
                thr = NR.centred_threshold(values, nominal)
                margin = NR.margin_to_threshold(values, thr)
                assert margin >= NR.EXACT_MARGIN, (K, mode, class_agnostic, nominal, margin)
                want = [NR.greedy_from_overlaps(c[4], c[5], ok, thr, K) for c, ok in zip(cases, oks)]
                got = device_nms(eng, box2d, box3d, cls, keep_in, mode, thr, class_agnostic)
                tag = (K, mode, class_agnostic, nominal, thr)
                assert_same(got, (np.stack([w[0] for w in want]), np.stack([w[1] for w in want])), tag)
                if K >= 63:     # the case has power: boxes are suppressed, others survive
                    assert 0 < int((got[1] >= 0).sum()) and int(got[0].sum()) > B, tag
                ran += 1
    assert ran == 12            # every generated case was tested, none skipped


# ------------------------------------------------------------------------------------------------ 3. K = 1024
@pytest.mark.parametrize("mode", [0, 1])
def test_k1024_everything_kept(eng, mode):
    """B = 2, K = 1024 participants per image -- the suppression matrix in the handle's workspace.  Clusters of 4 on a grid
    far wider than a box: the reference asks the oracle only for pairs closer than the sum of their half-diagonals."""
    B, K = 2, 1024
    imgs = [NR.grid_clusters(77 + b, K) for b in range(B)]
    box2d, box3d, cls, keep_in = (np.stack([im[i] for im in imgs]) for i in range(4))
    orders = [NR.participants_in_order(im[0][:, 4], im[3]) for im in imgs]
    ovs = [NR.ranked_overlaps(im[1], o, mode, near_only=True) for im, o in zip(imgs, orders)]
    ws0 = eng.workspace_bytes()
    for class_agnostic in (True, False):
        oks = [NR.compatible(im[2], o, class_agnostic) for im, o in zip(imgs, orders)]
        values = np.concatenate([ov[ok] for ov, ok in zip(ovs, oks)])
        thr = NR.centred_threshold(values, 0.3)
        assert NR.margin_to_threshold(values, thr) >= NR.EXACT_MARGIN
        want = [NR.greedy_from_overlaps(o, ov, ok, thr, K) for o, ov, ok in zip(orders, ovs, oks)]
        got = device_nms(eng, box2d, box3d, cls, keep_in, mode, thr, class_agnostic)
        assert_same(got, (np.stack([w[0] for w in want]), np.stack([w[1] for w in want])), (mode, class_agnostic, thr))
        assert int((got[1] >= 0).sum()) > 100 and int(got[0].sum()) > B * K // 4
    assert eng.workspace_bytes() >= max(ws0, B * K * (K // 64) * 8)     # the matrices are counted


# ------------------------------------------------------------------------------------------------ 4. ties and duplicates
@pytest.mark.parametrize("mode", [0, 1])
def test_ties_duplicates_and_degenerate_boxes(eng, mode):
    b = NR.closed_form_boxes()
    dup = np.stack([b[0]] * 3)
    # equal scores: the lower slot wins; bit-identical boxes have overlap 1 (suppressed below 1, kept AT 1: strict)
    assert check_single(eng, dup, [0.5, 0.5, 0.5], mode, 0.99) == ([1, 0, 0], [-1, 0, 0])
    assert check_single(eng, dup, [0.5, 0.7, 0.7], mode, 0.99) == ([0, 1, 0], [1, -1, 1])
    assert check_single(eng, dup, [0.5, 0.5, 0.5], mode, 1.0) == ([1, 1, 1], [-1, -1, -1])
    # the same ROTATED box twice (a pixel that peaks in two class channels): overlap 1, class-agnostic the weaker one dies
    rot = dup[:2].copy()
    rot[:, 6] = 0.3
    rot[:, 0] = -14.6
    assert check_single(eng, rot, [0.9, 0.8], mode, 0.99, cls=[0, 1], class_agnostic=True) == ([1, 0], [-1, 0])
    assert check_single(eng, rot, [0.8, 0.9], mode, 0.99, cls=[0, 1], class_agnostic=True) == ([0, 1], [1, -1])
    assert check_single(eng, rot, [0.9, 0.8], mode, 0.99, cls=[0, 1]) == ([1, 1], [-1, -1])
    # negative zero ranks below zero, and a negative score below both (the keys, not a float comparison)
    assert check_single(eng, dup, [-0.0, 0.0, -1.0], mode, 0.5) == ([0, 1, 0], [1, -1, 1])
    # a participant with zero dims -- inside another box or 30 m from it -- neither suppresses nor is suppressed
    z = np.stack([b[0]] * 3)
    z[1, 3:6] = 0
    z[2, 3:6] = 0
    z[2, 0] += 30
    for scores in ([0.9, 0.8, 0.7], [0.7, 0.8, 0.9]):
        assert check_single(eng, z, scores, mode, 0.0) == ([1, 1, 1], [-1, -1, -1])
    # a NaN overlap never suppresses
    nan = np.stack([b[0]] * 2)
    nan[1, 0] = np.nan
    for scores in ([0.9, 0.8], [0.8, 0.9]):
        assert check_single(eng, nan, scores, mode, 0.0) == ([1, 1], [-1, -1])
    nan[1] = np.nan
    assert check_single(eng, nan, [0.9, 0.8], mode, 0.0) == ([1, 1], [-1, -1])


# ------------------------------------------------------------------------------------------------ 5. masks and aliasing
def _raw_call(eng, t, B, K, mode, thr, class_agnostic, keep_out, by):
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(0)
    with torch.cuda.device(eng.device):
        return eng.lib.mc_nms3d(eng.h, p(t["box2d"]), p(t["box3d"]), p(t["cls"]), p(t["keep_thr"]), B, K, mode, thr,
                                class_agnostic, p(keep_out), p(by), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("mode", [0, 1])
def test_masks_and_aliasing(eng, mode):
    B, K = 3, 65
    cases = [NR.clustered_case(1000 * K + b, K, mode) for b in range(B)]
    box2d, box3d, cls, keep_in = (np.stack([c[i] for c in cases]) for i in range(4))
    oks = [NR.compatible(c[2], c[4], True) for c in cases]
    thr = NR.centred_threshold(np.concatenate([c[5][ok] for c, ok in zip(cases, oks)]), 0.3)
    # all-zero keep_in: nothing kept, nobody a participant
    gk, gb = device_nms(eng, box2d, box3d, cls, np.zeros_like(keep_in), mode, thr, True)
    assert not gk.any() and (gb == -2).all()
    # out of place (the reference's result, checked in test_clustered_random_boxes) ...
    gk, gb = device_nms(eng, box2d, box3d, cls, keep_in, mode, thr, True)
    want = [NR.greedy_from_overlaps(c[4], c[5], ok, thr, K) for c, ok in zip(cases, oks)]
    assert_same((gk, gb), (np.stack([w[0] for w in want]), np.stack([w[1] for w in want])), "out of place")
    # ... non-participants never appear as suppressors, and are marked -2
    part = keep_in != 0
    assert (gb[~part] == -2).all() and (gb[part] != -2).all() and not gk[~part].any()
    for i in range(B):
        s = gb[i][gb[i] >= 0]
        assert part[i][s].all() and gk[i][s].all()          # a suppressor is a KEPT participant
    # ... in place: keep_out is keep_in
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(eng.device)
    t = {"box2d": up(box2d, np.float32), "box3d": up(box3d, np.float32), "cls": up(cls, np.int64), "keep_thr": up(keep_in, np.uint8)}
    by = torch.full((B, K), 99, dtype=torch.int32, device=eng.device)
    assert _raw_call(eng, t, B, K, mode, thr, 1, t["keep_thr"], by) == 0
    assert np.array_equal(t["keep_thr"].cpu().numpy(), gk) and np.array_equal(by.cpu().numpy(), gb)
    # ... suppressed_by == NULL
    t["keep_thr"] = up(keep_in, np.uint8)
    out = torch.full((B, K), 9, dtype=torch.uint8, device=eng.device)
    assert _raw_call(eng, t, B, K, mode, thr, 1, out, None) == 0
    assert np.array_equal(out.cpu().numpy(), gk) and np.array_equal(t["keep_thr"].cpu().numpy(), keep_in)
    # Engine.nms3d's keep= overrides keep_thr
    o = eng.nms3d(t, thr, mode=MODES[mode], class_agnostic=True, keep=torch.zeros_like(t["keep_thr"]))
    assert not o["keep_nms"].any()


# ------------------------------------------------------------------------------------------------ 6. argument errors
def test_argument_errors_launch_nothing(eng):
    from hipmonocon import lib
    dev = eng.device
    B, K = 2, 8
    t = {"box2d": torch.rand(B, K, 5, device=dev), "box3d": torch.rand(B, K, 7, device=dev) + 1,
         "cls": torch.zeros(B, K, dtype=torch.int64, device=dev), "keep_thr": torch.ones(B, K, dtype=torch.uint8, device=dev)}
    big = {"box2d": torch.rand(1, 1025, 5, device=dev), "box3d": torch.rand(1, 1025, 7, device=dev) + 1,
           "cls": torch.zeros(1, 1025, dtype=torch.int64, device=dev), "keep_thr": torch.ones(1, 1025, dtype=torch.uint8, device=dev)}
    out = torch.full((B, 1025), 7, dtype=torch.uint8, device=dev)
    by = torch.full((B, 1025), 7, dtype=torch.int32, device=dev)
    bad = [(t, B, 0, 0, 0.5, "bad shape"), (big, 1, 1025, 0, 0.5, "bad shape"), (t, 0, K, 0, 0.5, "bad shape"),
           (t, B, K, 2, 0.5, "mode"), (t, B, K, -1, 0.5, "mode"), (t, B, K, 0, -0.1, "iou_thr"), (t, B, K, 1, 1.5, "iou_thr"),
           (t, B, K, 0, float("nan"), "iou_thr")]
    for src, b, k, mode, thr, word in bad:
        assert _raw_call(eng, src, b, k, mode, thr, 0, out, by) != 0, (b, k, mode, thr)
        assert word.encode() in eng.lib.mc_last_error(eng.h), (word, eng.lib.mc_last_error(eng.h))
    for missing in ("box2d", "box3d", "cls", "keep_thr"):
        assert _raw_call(eng, dict(t, **{missing: None}), B, K, 0, 0.5, 0, out, by) != 0
        assert b"null" in eng.lib.mc_last_error(eng.h)
    assert _raw_call(eng, t, B, K, 0, 0.5, 0, None, by) != 0 and b"null" in eng.lib.mc_last_error(eng.h)
    torch.cuda.synchronize()
    assert (out == 7).all() and (by == 7).all()                       # nothing was launched
    # the engine's wrapper: MonoconHipError from the library, from its own shape / dtype checks; ValueError for the mode
    for thr in (-0.1, 1.5, float("nan")):
        with pytest.raises(lib.MonoconHipError):
            eng.nms3d(t, thr)
    with pytest.raises(lib.MonoconHipError):
        eng.nms3d(big, 0.5)
    with pytest.raises(lib.MonoconHipError):
        eng.nms3d({k: v[:, :0] for k, v in t.items()}, 0.5)             # K = 0
    with pytest.raises(lib.MonoconHipError):
        eng.nms3d(dict(t, cls=t["cls"].int()), 0.5)
    with pytest.raises(lib.MonoconHipError):
        eng.nms3d(dict(t, keep_thr=t["keep_thr"][:1]), 0.5)
    with pytest.raises(ValueError):
        eng.nms3d(t, 0.5, mode="bogus")
    # and the valid call still works on this handle
    o = eng.nms3d(t, 0.5)
    assert o["keep_nms"].shape == (B, K) and bool(o["keep_nms"].any())


# ------------------------------------------------------------------------------------------------ 7. end to end
TOPK, THRES = 30, 0.4
CAR = (3.9, 1.6, 1.6)


def _planted_maps():
    """prediction maps of B = 2 images on a 24 x 80 feature map with planted near-duplicates: the same regressions two
    pixels apart in one class channel, and one pixel that peaks in two class channels (Pedestrian and Cyclist)"""
    from hipmonocon import synth
    d = synth.make_decode_inputs(31, 2, 24, 80, topk=TOPK)
    d = {k: v.copy() for k, v in d.items()}
    d["center_heatmap_pred"] *= np.float32(0.5)                          # the planted peaks are among the top 30

    def plant(b, c, y, x, heat, z, src=None):
        d["center_heatmap_pred"][b, c, y, x] = heat
        for k in ("wh_pred", "offset_pred", "center2kpt_offset_pred", "dim_pred", "depth_pred", "alpha_cls_pred", "alpha_offset_pred"):
            if src is not None:
                d[k][b, :, y, x] = d[k][b, :, src[0], src[1]]
        if src is None:
            d["wh_pred"][b, :, y, x] = 12.0
            d["offset_pred"][b, :, y, x] = 0.5
            d["center2kpt_offset_pred"][b, 16:18, y, x] = 0.25
            d["dim_pred"][b, :, y, x] = CAR
            d["depth_pred"][b, :, y, x] = (z, 0.0)          # sigma = exp(-0) = 1: the score is the heat value

    for b in range(2):
        d["center_heatmap_pred"][b, :, 8:19, 16:60] = 1e-4               # a quiet region for the planted peaks
        plant(b, 2, 10, 20, 0.95, 20.0 + b)
        plant(b, 2, 10, 22, 0.93, None, src=(10, 20))                    # two pixels apart, the same regressions
        plant(b, 0, 15, 50, 0.90, 12.0 + b)
        # the same pixel in another class channel: the same box twice (the header's rule gives the pair overlap 1; the
        # clipping of two bit-identical rotated boxes is round-off, and the oracle makes 1/3 of this pair)
        d["center_heatmap_pred"][b, 1, 15, 50] = 0.88
    return d


def _detector(sd, **nms):
    from model import MonoConDetector
    from model.detector.monocon_detector import default_test_config
    m = MonoConDetector(34, pretrained_backbone=False, test_config=dict(default_test_config, topk=TOPK, test_thres=THRES, **nms))
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _batch():
    from hipmonocon import synth
    batch = synth.make_batch(78, 2, 96, 320, with_labels=False)
    batch["img_metas"]["ori_shape"] = [(90, 310), (96, 320)]
    batch["img_metas"]["sample_idx"] = [5, 6]
    batch["img"] = batch["img"].cuda()
    return batch


def _plant(monkeypatch, m, maps):
    """the detector's forward hands out the planted maps (decode, NMS, formatting and the copies run as they are)"""
    eng = m._engine()
    monkeypatch.setattr(eng, "forward_infer", lambda img, want_feat=False: {k: v.clone() for k, v in maps.items()})
    return eng


def _filter_annos(annos, kept_scores):
    """the rows of a list of annotation dicts whose score is one of the image's kept scores"""
    out = []
    for a, s in zip(annos, kept_scores):
        sel = np.isin(np.asarray(a["score"], np.float32), s)
        out.append({k: np.asarray(v)[sel] for k, v in a.items()})
    return out


@pytest.fixture(scope="module")
def planted():
    maps = {k: torch.from_numpy(v).cuda() for k, v in _planted_maps().items()}
    return maps


def test_end_to_end_off_is_the_plain_decode(golden_sd, planted, monkeypatch):
    """without the keys: no keep_nms in the decode dict, its tensors bit-identical to a plain Engine.decode"""
    from hipmonocon import synth
    from hipmonocon.engine import p2_inverse
    m = _detector(golden_sd)
    eng = _plant(monkeypatch, m, planted)
    batch = _batch()
    R = m.head._decode_dense(batch, planted, eng)
    P2 = np.stack([synth.KITTI_P2] * 2).astype(np.float32)
    plain = eng.decode(planted, torch.from_numpy(P2).cuda(), torch.from_numpy(p2_inverse(P2)).cuda(), (96, 320), TOPK, THRES)
    assert set(R) == set(plain) == {"scores", "flat_index", "cls", "box2d", "box3d", "keep", "box_mask", "keep_thr"}
    for k in plain:
        assert (R[k] is None and plain[k] is None) or torch.equal(R[k], plain[k]), k
    # the planted peaks are there: both of the pair, and the pixel in both class channels
    for b in range(2):
        kept = R["keep_thr"][b].bool().cpu().numpy()
        sc = R["box2d"][b, :, 4].cpu().numpy()[kept]
        for s in (0.95, 0.93, 0.90, 0.88):
            assert np.isclose(sc, s, atol=1e-6).sum() == 1, (b, s)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("class_agnostic", [False, True])
def test_end_to_end_detect(golden_sd, planted, monkeypatch, mode, class_agnostic):
    """with nms_thres set, detect()'s annotation dicts are those of the NMS-off run filtered on the host by the reference;
    batch_eval(), detect() and detect_with_vis() agree; the decode dict gains keep_nms / suppressed_by"""
    off = _detector(golden_sd)
    _plant(monkeypatch, off, planted)
    with torch.no_grad():
        kitti_off, vis_off = off.detect_with_vis(_batch())
        R = off.head._decode_dense(_batch(), planted, off._engine())
    box2d, box3d = R["box2d"].cpu().numpy(), R["box3d"].cpu().numpy()
    cls, keep_thr = R["cls"].cpu().numpy(), R["keep_thr"].cpu().numpy()
    # the threshold: nominal 0.5, centred in the widest gap of the oracle's overlaps of the decoded boxes
    mode_id = MODES.index(mode)
    orders = [NR.participants_in_order(box2d[b][:, 4], keep_thr[b]) for b in range(2)]
    ovs = [NR.ranked_overlaps(box3d[b], orders[b], mode_id) for b in range(2)]
    oks = [NR.compatible(cls[b], orders[b], class_agnostic) for b in range(2)]
    values = np.concatenate([ov[ok] for ov, ok in zip(ovs, oks)])
    thr = NR.centred_threshold(values, 0.5)
    assert NR.margin_to_threshold(values, thr) >= NR.EXACT_MARGIN
    want = [NR.greedy_from_overlaps(orders[b], ovs[b], oks[b], thr, TOPK) for b in range(2)]
    keep_ref = np.stack([w[0] for w in want])
    # the planted duplicates: the pair in one channel always loses its weaker half, the two-channel pixel only class-agnostic
    for b in range(2):
        sc = box2d[b][:, 4]
        slot = lambda s: int(np.flatnonzero(np.isclose(sc, s, atol=1e-6) & (keep_thr[b] != 0))[0])
        assert keep_ref[b][slot(0.95)] == 1 and keep_ref[b][slot(0.93)] == 0 and want[b][1][slot(0.93)] == slot(0.95)
        assert keep_ref[b][slot(0.90)] == 1 and keep_ref[b][slot(0.88)] == (0 if class_agnostic else 1)
        kept_scores = sc[keep_thr[b] != 0]
        assert len(np.unique(kept_scores)) == len(kept_scores)          # rows are identified by their score below

    on = _detector(golden_sd, nms_thres=thr, nms_mode=mode, nms_class_agnostic=class_agnostic)
    _plant(monkeypatch, on, planted)
    with torch.no_grad():
        Rn = on.head._decode_dense(_batch(), planted, on._engine())
        kitti = on.detect(_batch())
        vis = on.detect(_batch(), get_vis_format=True)
        kitti2, vis2 = on.detect_with_vis(_batch())
        kitti_ref = on.batch_eval(_batch())
        vis_ref = on.batch_eval(_batch(), get_vis_format=True)
    # the decode dict
    assert set(Rn) == set(R) | {"keep_nms", "suppressed_by"}
    for k in ("scores", "flat_index", "cls", "box2d", "box3d", "keep_thr"):
        assert torch.equal(Rn[k], R[k]), k
    assert np.array_equal(Rn["keep_nms"].cpu().numpy(), keep_ref)
    assert np.array_equal(Rn["suppressed_by"].cpu().numpy(), np.stack([w[1] for w in want]))
    assert torch.equal(Rn["box_mask"], Rn["keep_nms"].bool())
    # detect() = the NMS-off run filtered on the host
    kept_scores = [box2d[b][keep_ref[b] != 0, 4] for b in range(2)]
    for field in ("img_bbox", "img_bbox2d"):
        exp = _filter_annos(kitti_off[field], kept_scores)
        assert sum(len(e["name"]) for e in exp) < sum(len(a["name"]) for a in kitti_off[field])
        for got in (kitti, kitti2):
            assert len(got[field]) == 2
            for a, e in zip(got[field], exp):
                assert set(a) == set(e)
                for k in e:
                    assert np.array_equal(np.asarray(a[k]), e[k]), (field, k)
    # the visualiser's list: the off run's boxes under the reference's mask, and the three entry points agree
    for b in range(2):
        sel = torch.from_numpy(keep_ref[b][keep_thr[b] != 0] != 0)
        for k in ("boxes_3d", "scores_3d", "labels_3d"):
            assert torch.equal(vis[b]["img_bbox"][k], vis_off[b]["img_bbox"][k][sel]), k
    _assert_vis_equal(vis, vis_ref)
    _assert_vis_equal(vis2, vis_ref)
    assert_annos_close(kitti["img_bbox"], kitti_ref["img_bbox"], "3d")
    assert_annos_close(kitti["img_bbox2d"], kitti_ref["img_bbox2d"], "2d")


def test_bad_mode_raises_before_any_launch(golden_sd, planted, monkeypatch):
    m = _detector(golden_sd, nms_thres=0.5, nms_mode="bogus")
    eng = _plant(monkeypatch, m, planted)
    calls = []
    monkeypatch.setattr(eng, "decode", lambda *a, **k: calls.append(1))
    with pytest.raises(ValueError):
        m.detect(_batch())
    assert not calls


def test_infer_raw_takes_the_nms_flags(golden_sd, tmp_path):
    """`infer_raw.py --nms_thres 0.1 --nms_mode 3d --nms_class_agnostic` over a 2-frame raw drive (batches of one, threshold
    0): the label files are those of a detector with the three test_config keys on the same frames, and shorter than
    those of a detector without them"""
    import os
    import subprocess
    import sys
    from conftest import PKG
    from dataset.kitti_raw_dataset import KITTIRawDataset
    from test_kitti_raw import make_raw_drive
    from utils.kitti_convert_utils import kitti_result_lines
    img_dir, calib = make_raw_drive(tmp_path / "drive", 2)
    ckpt, out = str(tmp_path / "seed7.pth"), str(tmp_path / "out")
    torch.save({"state_dict": {"model": golden_sd}}, ckpt)
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(PKG, "infer_raw.py"), "--data_dir", img_dir,
           "--calib_file", calib, "--checkpoint_file", ckpt, "--save_dir", out, "--batch_size", "1", "--num_workers", "1",
           "--test_thres", "0.0", "--nms_thres", "0.1", "--nms_mode", "3d", "--nms_class_agnostic"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])

    def parse(lines):
        rows = [ln.split() for ln in lines if ln.strip()]
        return [row[0] for row in rows], np.array([[float(v) for v in row[1:]] for row in rows]).reshape(len(rows), 15)

    from model import MonoConDetector
    from model.detector.monocon_detector import default_test_config
    cfg = dict(default_test_config, test_thres=0.0)
    dets = []
    for extra in (dict(nms_thres=0.1, nms_mode="3d", nms_class_agnostic=True), {}):
        m = MonoConDetector(34, pretrained_backbone=False, test_config=dict(cfg, **extra))
        m.load_state_dict(golden_sd, strict=True)
        dets.append(m.cuda().eval())
    ds = KITTIRawDataset(img_dir, calib)
    fewer = 0
    for i, path in enumerate(ds.image_files):
        with open(os.path.join(out, os.path.splitext(os.path.basename(path))[0] + ".txt")) as f:
            names, vals = parse(f.readlines())
        rows = []
        for m in dets:
            d = ds[i]
            d["img"] = d["img"].cuda()
            d["img_metas"]["ori_shape"] = [d["img_metas"]["ori_shape"][0][:2]]
            d["img_metas"]["sample_idx"] = [i]
            with torch.no_grad():
                rows.append(parse(kitti_result_lines(m.detect(d)["img_bbox"][0])))
        assert len(names) > 0 and names == rows[0][0], path
        assert np.allclose(vals, rows[0][1], rtol=1e-5, atol=2e-4), (path, float(np.abs(vals - rows[0][1]).max()))
        fewer += len(rows[1][0]) - len(names)
    assert fewer > 0
