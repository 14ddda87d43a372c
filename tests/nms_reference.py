"""The CPU reference of mc_nms3d (greedy 3D-box NMS after the decode) and the fixtures its tests share.

A plain module (no fixtures): `test_hip_nms3d.py` (the kernel, the engine and the detector on the device) and
`test_nms3d_host.py` (this reference checked against closed forms, without a device) share it.

The overlaps come from `oracle.kitti_eval_oracle.rotate_iou` (mode 0: bird's-eye-view IoU of (x, z, dim0, dim2, rot_y)) and
`box3d_overlap` (mode 1: 3D IoU of the box3d rows cast to double), both at criterion -1 and called as include/monocon_hip.h
states it: box = the higher-ranked participant, query = the lower-ranked one.  The greedy loop is the header's, and so are its
two additions, where the oracle's value is round-off and is not asked for:
  * a participant whose footprint has no area (dim0 or dim2 not > 0) overlaps nothing.  The IoU expression is a / (a - a) or
    0 / 0 for such a box (measured: 5.05 for a point-sized box inside a 4 x 2 m one, -8.4e6 for one 30 m away);
  * one footprint twice intersects in its own area (measured: the oracle gives less than 0.99 for 291 of 300 rotated boxes
    against themselves, 0 for many -- every vertex test is a tie).

Exactness.  The existing tests hold the device overlap to the oracle at 2e-5 .. 5e-5, so a keep mask can only be demanded bit
for bit when no oracle overlap of a participating, class-compatible pair lies within EXACT_MARGIN = 1e-3 of the threshold
(20x the pinned tolerance).  No case is dropped to get there: `centred_threshold` moves a nominal threshold to the centre of
the widest gap between consecutive oracle overlaps within +-0.05 of it, and asserts that the gap is at least 2e-3.
"""
import functools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "monocon-pytorch_amd")
for _p in (PKG, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import kitti_eval_oracle as KO      # noqa: E402

EXACT_MARGIN = 1e-3
MIN_GAP = 2e-3
BEV_COLS = [0, 2, 3, 5, 6]          # box3d (x, y, z, dim0, dim1, dim2, rot_y) -> the footprint (x, z, dim0, dim2, rot_y)


# ------------------------------------------------------------------------------------------------ order
def score_keys(scores):
    """the order-preserving uint32 image of float32 scores (kernels_decode.hip f2key): total for any bit pattern"""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def participants_in_order(scores, keep_in):
    """slots with keep_in != 0, by score descending (through the keys), ties by slot ascending"""
    slots = np.flatnonzero(np.asarray(keep_in) != 0)
    keys = score_keys(np.asarray(scores, dtype=np.float32)[slots])
    return slots[np.lexsort((slots, -keys.astype(np.int64)))]


# ------------------------------------------------------------------------------------------------ overlaps
def half_diagonals(box3d):
    b = np.asarray(box3d, dtype=np.float64)
    return 0.5 * np.hypot(b[:, 3], b[:, 5])


def ranked_overlaps(box3d, order, mode, near_only=False):
    """(n, n) float64, entry [i, j] for ranks i < j = ov(order[i], order[j]) from the oracle, 0 elsewhere.
    near_only: the oracle is only asked for pairs whose centres are closer than the sum of their half-diagonals (every
    corner of a box lies within its half-diagonal of its centre, so the other pairs do not meet) and 0 is taken for the rest."""
    box3d = np.asarray(box3d, dtype=np.float32)
    n = len(order)
    out = np.zeros((n, n), dtype=np.float64)
    if n < 2:
        return out
    b = box3d[order]
    hd = half_diagonals(b)
    cx, cz = b[:, 0].astype(np.float64), b[:, 2].astype(np.float64)
    with np.errstate(invalid="ignore"):
        has_area = (b[:, 3] > 0) & (b[:, 5] > 0)    # the header's addition: a footprint without area overlaps nothing
    for i in range(n - 1):
        if not has_area[i]:
            continue
        js = np.arange(i + 1, n)
        js = js[has_area[js]]
        if near_only:
            js = js[np.hypot(cx[js] - cx[i], cz[js] - cz[i]) < hd[js] + hd[i]]
        if not len(js):
            continue
        if mode == 0:
            out[i, js] = KO.rotate_iou(b[i:i + 1, BEV_COLS], b[js][:, BEV_COLS], -1)[0]
        else:
            out[i, js] = KO.box3d_overlap(b[i:i + 1].astype(np.float64), b[js].astype(np.float64), -1)[0]
        # the header's other addition: one footprint twice intersects in its own area (the oracle's vertex tests are all
        # ties there -- it gives less than 0.99 for 291 of 300 rotated boxes of clustered_boxes against themselves)
        for j in js[(b[js][:, BEV_COLS] == b[i, BEV_COLS]).all(1)]:
            out[i, j] = _overlap_from_area(np.float32(b[i, 3] * b[i, 5]), b[i], b[j], mode)
    return out


def _overlap_from_area(area, bi, bj, mode):
    """criterion -1 of rotate_iou.py:252-277 (mode 0) / eval.py:128-157 (mode 1) for a given float32 intersection area"""
    ai = np.float64(area)
    if mode == 0:
        return float(np.float32(ai / (np.float64(np.float32(np.float32(bj[3] * bj[5]) + np.float32(bi[3] * bi[5]))) - ai)))
    bi, bj = bi.astype(np.float64), bj.astype(np.float64)
    iw = min(bi[1], bj[1]) - max(bi[1] - bi[4], bj[1] - bj[4])
    if not (area > 0 and iw > 0):
        return 0.0
    inc = iw * ai
    return float(inc / (bi[3] * bi[4] * bi[5] + bj[3] * bj[4] * bj[5] - inc))


def compatible(cls, order, class_agnostic):
    """(n, n) bool over ranks: may the pair suppress at all (i < j and the class condition)"""
    c = np.asarray(cls)[order]
    ok = np.ones((len(order), len(order)), dtype=bool) if class_agnostic else (c[:, None] == c[None, :])
    return np.triu(ok, 1)


# ------------------------------------------------------------------------------------------------ threshold
def centred_threshold(values, nominal, half_window=0.05):
    """the float32 threshold at the centre of the widest gap between consecutive `values` within +-half_window of nominal
    (the window's ends count as values); the gap must be at least MIN_GAP"""
    v = np.asarray(values, dtype=np.float64)
    lo, hi = max(nominal - half_window, 0.0), min(nominal + half_window, 1.0)
    pts = np.sort(np.concatenate([[lo, hi], v[np.isfinite(v) & (v > lo) & (v < hi)]]))
    gaps = np.diff(pts)
    k = int(np.argmax(gaps))
    assert gaps[k] >= MIN_GAP, (nominal, float(gaps[k]))
    return float(np.float32(0.5 * (pts[k] + pts[k + 1])))


def margin_to_threshold(values, thr):
    """smallest |value - thr| over the finite values (inf when there are none)"""
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    return float(np.abs(v - thr).min()) if v.size else float("inf")


# ------------------------------------------------------------------------------------------------ the greedy pass
def greedy_from_overlaps(order, ov, ok, thr, K):
    """keep_out (K,) uint8 and suppressed_by (K,) int32 from ranked overlaps `ov`, the compatibility mask `ok` and thr"""
    thr = np.float32(thr)
    n = len(order)
    keep = np.zeros(K, dtype=np.uint8)
    by = np.full(K, -2, dtype=np.int32)
    alive = np.ones(n, dtype=bool)
    with np.errstate(invalid="ignore"):
        hit = ok & (ov > np.float64(thr))           # strict; a NaN overlap compares false
    for i in range(n):
        if not alive[i]:
            continue                                # a box that was itself suppressed suppresses nothing
        keep[order[i]] = 1
        by[order[i]] = -1
        for j in np.flatnonzero(hit[i] & alive):
            if j > i:
                alive[j] = False
                by[order[j]] = order[i]
    return keep, by


def nms_reference(box2d, box3d, cls, keep_in, mode, thr, class_agnostic, near_only=False):
    """one image: (keep_out, suppressed_by, the oracle overlaps of the participating class-compatible pairs)"""
    order = participants_in_order(np.asarray(box2d)[:, 4], keep_in)
    ov = ranked_overlaps(box3d, order, mode, near_only)
    ok = compatible(cls, order, class_agnostic)
    keep, by = greedy_from_overlaps(order, ov, ok, thr, len(keep_in))
    return keep, by, ov[ok]


# ------------------------------------------------------------------------------------------------ fixtures
def clustered_boxes(seed, K, n_centres=12, keep_frac=0.8):
    """K decoded boxes of one image around n_centres cluster centres: x in [-20, 20], y in [1, 2], z in [5, 60], dims
    l in [3.2, 4.6], h in [1.4, 1.8], w in [1.5, 1.9], rot_y uniform; a box = its centre + N(0, (0.5, 0.1, 0.8)) m, dims times
    U(0.9, 1.1), rot_y + N(0, 0.15).  -> box2d (K,5) (only the score column matters), box3d (K,7), cls (K,) int64 in
    0..2, keep_in (K,) uint8 (~keep_frac ones)."""
    rng = np.random.default_rng(seed)
    cen = np.stack([rng.uniform(-20, 20, n_centres), rng.uniform(1, 2, n_centres), rng.uniform(5, 60, n_centres)], 1)
    dims = np.stack([rng.uniform(3.2, 4.6, n_centres), rng.uniform(1.4, 1.8, n_centres), rng.uniform(1.5, 1.9, n_centres)], 1)
    rot = rng.uniform(-np.pi, np.pi, n_centres)
    which = rng.integers(0, n_centres, K)
    box3d = np.zeros((K, 7), dtype=np.float64)
    box3d[:, :3] = cen[which] + rng.normal(0, 1, (K, 3)) * np.array([0.5, 0.1, 0.8])
    box3d[:, 3:6] = dims[which] * rng.uniform(0.9, 1.1, (K, 3))
    box3d[:, 6] = rot[which] + rng.normal(0, 0.15, K)
    box2d = rng.uniform(0, 1000, (K, 5)).astype(np.float32)
    box2d[:, 4] = rng.permutation(np.linspace(0.05, 0.99, K)).astype(np.float32)      # distinct scores
    cls = rng.integers(0, 3, K).astype(np.int64)
    keep_in = (rng.uniform(0, 1, K) < keep_frac).astype(np.uint8)
    return box2d, box3d.astype(np.float32), cls, keep_in


def grid_clusters(seed, K=1024, per_cluster=4, pitch=15.0):
    """K boxes, everything kept: clusters of per_cluster on a square grid of `pitch` metres -- far wider than a box (half
    diagonal < 2.6 m, offsets below 4 m), so that only pairs of one cluster can overlap.  With 6 pairs per cluster and
    K / 4 clusters the overlaps must leave room for a threshold: the members of a cluster are near-duplicates (a quarter of
    clustered_boxes' jitter: overlaps mostly above 0.6), and in every other cluster the second half of the members stands
    3 m to the side of the first (overlaps mostly 0)."""
    rng = np.random.default_rng(seed)
    nc = K // per_cluster
    side = int(np.ceil(np.sqrt(nc)))
    which = np.repeat(np.arange(nc), per_cluster)
    member = np.tile(np.arange(per_cluster), nc)
    gx, gz = (which % side - side / 2.0) * pitch, 5.0 + (which // side) * pitch
    dims = np.stack([rng.uniform(3.2, 4.6, nc), rng.uniform(1.4, 1.8, nc), rng.uniform(1.5, 1.9, nc)], 1)
    rot = rng.uniform(-np.pi, np.pi, nc)
    aside = 3.0 * ((which % 2 == 1) & (member >= per_cluster // 2))
    box3d = np.zeros((K, 7), dtype=np.float64)
    box3d[:, 0] = gx + rng.normal(0, 0.125, K) + aside * np.cos(rot[which] + np.pi / 2)
    box3d[:, 1] = 1.5 + rng.normal(0, 0.025, K)
    box3d[:, 2] = gz + rng.normal(0, 0.2, K) - aside * np.sin(rot[which] + np.pi / 2)
    box3d[:, 3:6] = dims[which] * rng.uniform(0.9, 1.1, (K, 3))
    box3d[:, 6] = rot[which] + rng.normal(0, 0.04, K)
    perm = rng.permutation(K)                       # slots are not in cluster order
    box2d = rng.uniform(0, 1000, (K, 5)).astype(np.float32)
    box2d[:, 4] = rng.permutation(np.linspace(0.05, 0.99, K)).astype(np.float32)
    cls = rng.integers(0, 3, K).astype(np.int64)
    return box2d, box3d[perm].astype(np.float32), cls, np.ones(K, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def clustered_case(seed, K, mode):
    """a clustered image and its ranked oracle overlaps, computed once and shared (read-only) by every threshold / class
    setting of the tests"""
    box2d, box3d, cls, keep_in = clustered_boxes(seed, K)
    order = participants_in_order(box2d[:, 4], keep_in)
    ov = ranked_overlaps(box3d, order, mode)
    for a in (box2d, box3d, cls, keep_in, order, ov):
        a.setflags(write=False)
    return box2d, box3d, cls, keep_in, order, ov


def closed_form_boxes():
    """A, B, C: axis-aligned (rot_y = 0), l = 4, w = 2, equal height and y, at x = 0, 1, 2: IoU(A,B) = IoU(B,C) = 0.6 and
    IoU(A,C) = 1/3 in both modes.  D: C's footprint, but above the others with no height in common (y is the bottom face
    and points down; heights span [y - h, y])."""
    box3d = np.array([[0, 1.5, 20, 4, 1.5, 2, 0], [1, 1.5, 20, 4, 1.5, 2, 0], [2, 1.5, 20, 4, 1.5, 2, 0],
                      [2, -1.0, 20, 4, 1.5, 2, 0]], dtype=np.float32)
    return box3d
