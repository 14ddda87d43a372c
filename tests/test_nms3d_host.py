"""The host side of the opt-in 3D-box NMS, without a device: the CPU reference of the greedy pass (tests/nms_reference.py)
against closed forms, the test_config keys of the head, the unchanged default config dicts, the header's declaration."""
import os
import re

import numpy as np
import pytest
import torch

import nms_reference as NR
from conftest import REPO


def _run(box3d, scores, mode, thr, cls=None, keep_in=None, class_agnostic=False):
    K = len(box3d)
    box2d = np.zeros((K, 5), dtype=np.float32)
    box2d[:, 4] = scores
    cls = np.zeros(K, dtype=np.int64) if cls is None else np.asarray(cls, dtype=np.int64)
    keep_in = np.ones(K, dtype=np.uint8) if keep_in is None else np.asarray(keep_in, dtype=np.uint8)
    keep, by, _ = NR.nms_reference(box2d, box3d, cls, keep_in, mode, thr, class_agnostic)
    return keep.tolist(), by.tolist()


@pytest.mark.parametrize("mode", [0, 1])
def test_reference_closed_forms(mode):
    """A, B, C at x = 0, 1, 2 (l = 4, w = 2): IoU(A,B) = IoU(B,C) = 0.6, IoU(A,C) = 1/3, threshold 0.5"""
    abc = NR.closed_form_boxes()[:3]
    ov = NR.ranked_overlaps(abc, np.arange(3), mode)
    assert np.allclose(ov[0, 1], 0.6, atol=1e-6) and np.allclose(ov[1, 2], 0.6, atol=1e-6) and np.allclose(ov[0, 2], 1 / 3, atol=1e-6)
    # scores A > B > C: A kills B, and the dead B must not kill C
    assert _run(abc, [0.9, 0.8, 0.7], mode, 0.5) == ([1, 0, 1], [-1, 0, -1])
    # scores B > A > C: only B is kept
    assert _run(abc, [0.8, 0.9, 0.7], mode, 0.5) == ([0, 1, 0], [1, -1, 1])
    # classes: B of another class survives A, and then suppresses nothing of A's class; class-agnostic it dies as before
    assert _run(abc, [0.9, 0.8, 0.7], mode, 0.5, cls=[0, 1, 0]) == ([1, 1, 1], [-1, -1, -1])
    assert _run(abc, [0.9, 0.8, 0.7], mode, 0.5, cls=[0, 1, 0], class_agnostic=True) == ([1, 0, 1], [-1, 0, -1])
    # a non-participant neither suppresses nor is kept
    assert _run(abc, [0.9, 0.8, 0.7], mode, 0.5, keep_in=[0, 1, 1]) == ([0, 1, 0], [-2, -1, 1])


def test_reference_height_only_matters_in_3d():
    """D has C's footprint and no height in common with it: it dies in mode 0 and survives in mode 1"""
    b = NR.closed_form_boxes()
    assert _run(b[2:], [0.9, 0.8], 0, 0.5) == ([1, 0], [-1, 0])
    assert _run(b[2:], [0.9, 0.8], 1, 0.5) == ([1, 1], [-1, -1])


def test_reference_ties_duplicates_and_degenerate_boxes():
    b = NR.closed_form_boxes()
    dup = np.stack([b[0], b[0], b[0]])
    for mode in (0, 1):
        assert NR.ranked_overlaps(dup, np.arange(3), mode)[0, 1] == 1.0                 # bit-identical boxes
        assert _run(dup, [0.5, 0.5, 0.5], mode, 0.99) == ([1, 0, 0], [-1, 0, 0])        # equal scores: the lower slot wins
        assert _run(dup, [0.5, 0.7, 0.7], mode, 0.99) == ([0, 1, 0], [1, -1, 1])
        assert _run(dup, [0.5, 0.5, 0.5], mode, 1.0)[0] == [1, 1, 1]                    # strict: an overlap AT the threshold stays
        # the same ROTATED box twice (a pixel that peaks in two class channels): overlap 1 by the header's rule, whatever
        # the clipping makes of its ties
        rot = dup[:2].copy()
        rot[:, 6] = 0.3
        rot[:, 0] = -14.6
        assert abs(NR.ranked_overlaps(rot, np.arange(2), mode)[0, 1] - 1.0) < 1e-6
        assert _run(rot, [0.9, 0.8], mode, 0.99, cls=[0, 1], class_agnostic=True) == ([1, 0], [-1, 0])
        assert _run(rot, [0.9, 0.8], mode, 0.99, cls=[0, 1]) == ([1, 1], [-1, -1])
        # a participant with zero dims, inside another box or far from it, neither suppresses nor is suppressed
        z = np.stack([b[0], b[0], b[0]])
        z[1, 3:6] = 0
        z[2, 3:6] = 0
        z[2, 0] += 30
        for scores in ([0.9, 0.8, 0.7], [0.7, 0.8, 0.9]):
            assert _run(z, scores, mode, 0.0) == ([1, 1, 1], [-1, -1, -1])
        # a NaN overlap never suppresses
        nan = np.stack([b[0], b[0]])
        nan[1, 0] = np.nan
        assert _run(nan, [0.9, 0.8], mode, 0.0) == ([1, 1], [-1, -1])


def test_score_keys_are_a_total_order():
    s = np.array([np.nan, np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf], dtype=np.float32)
    k = NR.score_keys(s)
    assert len(set(k.tolist())) == len(s) and (np.diff(k[1:].astype(np.int64)) < 0).all()
    order = NR.participants_in_order(np.array([0.5, np.nan, 0.5, 0.7], np.float32), np.array([1, 1, 1, 0]))
    assert order.tolist() == [1, 0, 2]          # a positive NaN's bit pattern ranks above every number; ties by slot


def test_near_only_shortcut_skips_only_zero_overlaps():
    """pairs whose centres are at least the sum of the half-diagonals apart: the oracle gives exactly 0 for each of them"""
    box2d, box3d, cls, keep_in = NR.clustered_boxes(148, 48)
    order = NR.participants_in_order(box2d[:, 4], keep_in)
    for mode in (0, 1):
        full, near = NR.ranked_overlaps(box3d, order, mode), NR.ranked_overlaps(box3d, order, mode, near_only=True)
        assert np.array_equal(full, near) and (full > 0).sum() > 20
        assert np.isfinite(full).all()


def test_centred_threshold_keeps_the_margin():
    v = np.array([0.2, 0.27, 0.298, 0.3005, 0.301, 0.34, 0.6])
    thr = NR.centred_threshold(v, 0.3)
    assert abs(thr - 0.3205) < 1e-6 and NR.margin_to_threshold(v, thr) >= NR.EXACT_MARGIN
    with pytest.raises(AssertionError):
        NR.centred_threshold(np.linspace(0.25, 0.35, 101), 0.3)


def _head(**cfg):
    from model.dense_heads import MonoConDenseHeads
    from model.dense_heads.monocon_heads import DEFAULT_TEST_CFG
    return MonoConDenseHeads(test_config=dict(DEFAULT_TEST_CFG, **cfg))


def test_head_reads_the_three_keys_and_rejects_a_bad_mode():
    """the mode string is checked when the decode is reached (not in the constructor), before any launch: no device, no
    calibration and no engine is touched on the way"""
    assert _head()._nms_config() is None
    assert _head(nms_thres=None, nms_mode='bogus')._nms_config() is None           # off: the other keys are not read
    assert _head(nms_thres=0.5)._nms_config() == dict(thres=0.5, mode='bev', class_agnostic=False)
    assert _head(nms_thres=0.25, nms_mode='3d', nms_class_agnostic=True)._nms_config() == dict(thres=0.25, mode='3d',
                                                                                             class_agnostic=True)
    head = _head(nms_thres=0.5, nms_mode='bogus')                                   # the constructor accepts it
    data = {'img_metas': {'pad_shape': [(96, 320)]}}
    pred = {'center_heatmap_pred': torch.zeros(1, 3, 24, 80)}
    with pytest.raises(ValueError, match="bogus"):
        head._decode_dense(data, pred)
    with pytest.raises(ValueError, match="bogus"):
        head.decode_heatmap(data, pred)


def test_scripts_offer_the_flags():
    """test.py and infer_raw.py (which runs test_raw.py's main and hands its detector the keys) take --nms_thres, --nms_mode
    and --nms_class_agnostic; the head carries no setting outside its own test_config"""
    from model.dense_heads import MonoConDenseHeads
    assert not hasattr(MonoConDenseHeads, "test_config_overlay")
    from conftest import PKG
    for script in ("test.py", "infer_raw.py"):
        src = open(os.path.join(PKG, script)).read()
        for flag in ("'--nms_thres'", "'--nms_mode'", "'--nms_class_agnostic'"):
            assert flag in src, (script, flag)


def test_default_config_dicts_are_unchanged():
    from model.dense_heads.monocon_heads import DEFAULT_TEST_CFG
    from model.detector.monocon_detector import default_test_config
    want = {'topk': 30, 'local_maximum_kernel': 3, 'max_per_img': 30, 'test_thres': 0.4}
    assert DEFAULT_TEST_CFG == want and default_test_config == want


def test_engine_mode_names():
    from hipmonocon.engine import nms_mode_id
    assert nms_mode_id('bev') == 0 and nms_mode_id('3d') == 1
    for bad in ('BEV', '', None, 0):
        with pytest.raises(ValueError):
            nms_mode_id(bad)


def test_header_declares_mc_nms3d():
    txt = open(os.path.join(REPO, "include", "monocon_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"int\s+mc_nms3d\s*\(([^)]*)\)\s*;", code)
    assert m, "include/monocon_hip.h does not declare mc_nms3d"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 13 and args[0].startswith("mc_handle") and args[-1].startswith("void")
    assert "float iou_thr" in args and "int class_agnostic" in args and "int *suppressed_by" in args
    from hipmonocon import lib
    assert "mc_nms3d" in lib.EXPORTS
