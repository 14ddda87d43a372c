#!/usr/bin/env python
"""Golden vectors for the rotated-box overlap kernels from the REFERENCE'S OWN rotated-IoU code:
engine/kitti_eval/rotate_iou.py (the numba.cuda kernel ``rotate_iou_kernel_eval``, its device functions and its host
wrapper ``rotate_iou_gpu_eval``) and the BEV / 3D paths of engine/kitti_eval/eval.py that call it.

Runs only where the reference tree is available (read-only); the tests read ``rotate_iou_ref.npz`` and
``meta_rotate_iou.json``.  It imports make_f4_golden.py for its placeholders (cv2) and path set-up, then replaces the
numba placeholder with an EXECUTING shim and re-imports the reference's evaluator under it:

  * ``numba.jit`` / ``cuda.jit(device=True)``: identity decorators -- the device functions run as plain Python.
  * ``numba.float32`` is ``DT`` and ``cuda.local.array(shape, dtype)`` is ``np.zeros(shape, DT)``, with ``DT`` selectable:
      ref32 -- DT = float32, the storage the reference declares;
      ref64 -- DT = float64, the same algorithm at high precision (inputs are the same float32 values).
    A write past the 16-float vertex buffer raises IndexError in numpy, so the reference's undefined overrun (more than
    8 candidate vertices) is detected and recorded instead of silently corrupting memory.
  * ``cuda.jit(signature, ...)`` returns a launchable kernel: ``kernel[grid, block, stream](...)`` runs every block of the
    grid with one Python thread per CUDA thread, ``cuda.blockIdx`` / ``cuda.threadIdx`` through ``threading.local``,
    ``cuda.shared.array`` cached per block and ``cuda.syncthreads`` as a ``threading.Barrier``.  With stand-ins for
    ``cuda.select_device``, ``cuda.stream`` and ``cuda.to_device`` / ``copy_to_host`` on numpy arrays, the reference's
    ``rotate_iou_gpu_eval`` runs unchanged, also inside its ``bev_box_overlap`` and ``d3_box_overlap``.

Outputs: a labelled pair catalogue (inputs, ref32 / ref64 for the four criteria, candidate-vertex counts, overrun flags,
stability mask, closed forms), the emulated kernel on 70 x 131 matrices, 3D overlaps, and an end-to-end ``kitti_eval``.
The script is deterministic: two runs write equal arrays.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_rotate_iou_golden.py
"""
import contextlib
import json
import math
import os
import sys
import threading
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_f4_golden as F4                                 # noqa: E402  (cv2 placeholder, sys.path, save())
import numpy as np                                          # noqa: E402

# ------------------------------------------------------------------------------------------------ executing numba shim
STATE = types.SimpleNamespace(dt=np.float32, widen=False)
_TLS = threading.local()


class _Dim3:
    def __init__(self, x=0, y=0, z=0):
        self.x, self.y, self.z = x, y, z


def _local_array(shape, dtype=None):
    # every local array of the reference is declared numba.float32 == DT; widened mode gives the 16-float buffers room
    # for all candidates (what the reference's algorithm would compute without the overrun)
    if STATE.widen and shape in ((16,), 16):
        shape = (64,)
    return np.zeros(shape, STATE.dt)


def _shared_array(shape, dtype=None):
    cache = _TLS.shared
    key = (_TLS.shared_ctr,)
    _TLS.shared_ctr += 1
    with _TLS.lock:
        if key not in cache:
            cache[key] = np.zeros(shape, STATE.dt)
        return cache[key]


class _Kernel:
    """cuda.jit(signature)(fn): kernel[grid, block, stream](*args) runs the grid block by block, a thread per lane"""
    def __init__(self, fn):
        self.fn = fn

    def __getitem__(self, cfg):
        grid, block = cfg[0], cfg[1]
        grid = tuple(grid) if isinstance(grid, tuple) else (grid,)
        grid = grid + (1,) * (3 - len(grid))
        nthr = int(block)

        def launch(*args):
            for bz in range(grid[2]):
                for by in range(grid[1]):
                    for bx in range(grid[0]):
                        self._block((bx, by, bz), nthr, args)
        return launch

    def _block(self, bidx, nthr, args):
        barrier, shared, lock, errors = threading.Barrier(nthr), {}, threading.Lock(), []

        def lane(t):
            _TLS.block, _TLS.thread = _Dim3(*bidx), _Dim3(t)
            _TLS.barrier, _TLS.shared, _TLS.shared_ctr, _TLS.lock = barrier, shared, 0, lock
            try:
                self.fn(*args)
            except BaseException as e:          # noqa: BLE001 -- re-raised by the launcher
                errors.append(e)
                barrier.abort()
        threads = [threading.Thread(target=lane, args=(t,)) for t in range(nthr)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        if errors:
            raise errors[0]


class _DeviceArray(np.ndarray):
    def copy_to_host(self, ary=None, stream=None):
        if ary is None:
            return np.array(self)
        ary[...] = self
        return ary


class _Stream:
    @contextlib.contextmanager
    def auto_synchronize(self):
        yield self


class _CudaShim(types.ModuleType):
    blockIdx = property(lambda self: _TLS.block)
    threadIdx = property(lambda self: _TLS.thread)

    def __init__(self):
        super().__init__("numba.cuda")
        self.local = types.SimpleNamespace(array=_local_array)
        self.shared = types.SimpleNamespace(array=_shared_array)

    @staticmethod
    def jit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        if kwargs.get("device"):
            return lambda fn: fn
        return _Kernel                       # a signature: the decorated function becomes a launchable kernel

    @staticmethod
    def syncthreads():
        _TLS.barrier.wait()

    @staticmethod
    def select_device(device_id):
        return device_id

    @staticmethod
    def stream():
        return _Stream()

    @staticmethod
    def to_device(ary, stream=None):
        return np.array(ary, copy=True).view(_DeviceArray)


class _NumbaShim(types.ModuleType):
    float32 = property(lambda self: STATE.dt)

    def __init__(self, cuda):
        super().__init__("numba")
        self.__path__ = []
        self.cuda = cuda
        self.prange = range

    @staticmethod
    def jit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda fn: fn


SHIM = {"numba.jit": "identity decorator", "numba.prange": "builtins.range",
        "numba.float32": "DT (float32 for ref32, float64 for ref64)",
        "cuda.jit(device=True)": "identity decorator: the device functions run as plain Python",
        "cuda.jit(signature)": "launchable kernel: kernel[grid, block, stream] runs each block with one Python thread per "
                               "lane (threading.local blockIdx / threadIdx, shared arrays cached per block, syncthreads = "
                               "threading.Barrier(block))",
        "cuda.local.array(shape, dtype)": "np.zeros(shape, DT): an out-of-bounds write raises IndexError (overrun flag)",
        "cuda.select_device / stream / to_device / copy_to_host": "no-op device, numpy arrays"}

NUMPY2_TYPING = [
    "trangle_area: float32 / 2.0 stays float32 under NEP 50 (numba: float64); exact either way, a halving",
    "area(): the accumulator area_val = 0.0 is a Python float; += float32 gives float32 under NEP 50 (numba: float64 sum)",
    "devRotateIoUEval: area_inter / (area1 + area2 - area_inter) therefore in float32 (numba: float64, stored as float32)",
    "sort_vertex_in_convex_polygon: center /= num_of_inter is float32 / int -> float32 (numba: float64, stored float32; "
    "the same value, double rounding of a division is innocuous)",
    "math.cos / math.sin / math.sqrt on float32 return a double that NEP 50 rounds to float32 at its first use (numba: "
    "cosf / sinf / sqrtf; sqrt identical, cos / sin within an ulp)",
]

sys.modules["numba"] = _NumbaShim(_CudaShim())
sys.modules["numba.cuda"] = sys.modules["numba"].cuda
for m in [m for m in sys.modules if m == "engine" or m.startswith(("engine.", "kitti_eval"))]:
    del sys.modules[m]                     # make_f4_golden imported the evaluator under the inert placeholder
import engine.kitti_eval.rotate_iou as RR   # noqa: E402  (reference)
from engine.kitti_eval import eval as RE    # noqa: E402  (reference)
from hipmonocon import synth                # noqa: E402  (this repo)

assert RR.__file__.startswith("/root/reference/") and RE.__file__.startswith("/root/reference/")
RE_ROT = sys.modules["kitti_eval.rotate_iou"]           # eval.py's own import of rotate_iou (its d3_box_overlap uses it)
assert RE_ROT.__file__.startswith("/root/reference/") and isinstance(RE_ROT.rotate_iou_kernel_eval, _Kernel)

CRITERIA = (-1, 0, 1, 2)


# ------------------------------------------------------------------------------------------------ per-pair evaluation
def ref_pair(q, b, crit, dt):
    """devRotateIoUEval(q, b, crit) at storage DT; (value, overrun).  On an overrun the value is NaN."""
    STATE.dt = dt
    with np.errstate(all="ignore"):
        try:
            return float(RR.devRotateIoUEval(np.asarray(q, dt), np.asarray(b, dt), crit)), False
        except IndexError:
            return float("nan"), True


def ref_pair_wide(q, b, crit):
    """the reference's algorithm at float32 with vertex buffers wide enough for every candidate"""
    STATE.dt, STATE.widen = np.float32, True
    try:
        with np.errstate(all="ignore"):
            return float(RR.devRotateIoUEval(np.asarray(q, np.float32), np.asarray(b, np.float32), crit))
    finally:
        STATE.widen = False


def candidates(q, b, dt):
    """number of candidate vertices quadrilateral_intersection collects (rbox1 = the query), in a 64-float buffer"""
    STATE.dt = dt
    c1, c2 = np.zeros(8, dt), np.zeros(8, dt)
    RR.rbbox_to_corners(c1, np.asarray(q, dt))
    RR.rbbox_to_corners(c2, np.asarray(b, dt))
    with np.errstate(all="ignore"):
        return int(RR.quadrilateral_intersection(c1, c2, np.zeros(64, dt)))


# ------------------------------------------------------------------------------------------------ pair catalogue
CLASSES = ["generic", "kitti", "disjoint", "nested", "exact_aa", "near_copy", "turned_copy", "exact_copy",
           "far_pedestrian", "wide_angle", "dontcare", "zero_area"]
CAR, PED, CYC = ((3.2, 4.8), (1.5, 2.0)), ((0.5, 1.0), (0.4, 0.8)), ((1.5, 1.9), (0.5, 0.8))


def random_rboxes(rng, n, spread=6.0):
    """tests/test_kitti_eval.py's distribution"""
    return np.stack([rng.uniform(-spread, spread, n), rng.uniform(10, 10 + 2 * spread, n), rng.uniform(0.5, 5.0, n),
                     rng.uniform(0.5, 2.5, n), rng.uniform(-math.pi, math.pi, n)], axis=1)


def kitti_labels(rng, n, dims=None, z=(2.0, 80.0)):
    """bird's-eye-view label boxes (x, z, l, w, ry) of mixed classes at KITTI scale"""
    out = np.zeros((n, 5))
    for i in range(n):
        (l0, l1), (w0, w1) = dims or (CAR, PED, CYC)[int(rng.integers(0, 3))]
        out[i] = [rng.uniform(-40, 40), rng.uniform(*z), rng.uniform(l0, l1), rng.uniform(w0, w1), rng.uniform(-math.pi, math.pi)]
    return out


def detections(rng, lab, scale):
    """noisy detections of the labels: position noise in units of the box width, dims and heading jitter"""
    n = len(lab)
    d = lab.copy()
    s = np.asarray(scale, dtype=np.float64).reshape(-1, 1) if np.ndim(scale) else np.full((n, 1), scale)
    d[:, :2] += rng.normal(0, 1, (n, 2)) * s * lab[:, 3:4]
    d[:, 2:4] *= np.exp(rng.normal(0, 0.5, (n, 2)) * s)
    d[:, 4] += rng.normal(0, 0.6, n) * s[:, 0]
    return d


def catalogue(rng):
    """-> (q (M,5), b (M,5), class index (M,), exact (M,4) closed forms or NaN)"""
    Q, B, C, X = [], [], [], []

    def add(cls, q, b, exact=None):
        q, b = np.asarray(q, np.float64).reshape(-1, 5), np.asarray(b, np.float64).reshape(-1, 5)
        Q.append(q); B.append(b); C.append(np.full(len(q), CLASSES.index(cls)))
        X.append(np.full((len(q), 4), np.nan) if exact is None else np.asarray(exact, np.float64).reshape(-1, 4))

    add("generic", random_rboxes(rng, 2000), random_rboxes(rng, 2000))
    lab = kitti_labels(rng, 3000)
    add("kitti", detections(rng, lab, rng.choice([0.15, 0.3, 0.55], 3000)), lab)       # IoU around 0.7 / 0.5 / 0.25

    # disjoint: centres farther apart than the two half diagonals
    a, b = kitti_labels(rng, 800), kitti_labels(rng, 800)
    reach = 0.5 * (np.hypot(a[:, 2], a[:, 3]) + np.hypot(b[:, 2], b[:, 3]))
    ang = rng.uniform(-math.pi, math.pi, 800)
    dist = reach * rng.uniform(1.02, 4.0, 800) + rng.uniform(0, 30, 800) * (rng.uniform(size=800) < 0.3)
    b[:, 0], b[:, 1] = a[:, 0] + dist * np.cos(ang), a[:, 1] + dist * np.sin(ang)
    add("disjoint", a, b, np.zeros((800, 4)))

    # nested: a small box turned freely strictly inside a big one (the inner disk of the outer box holds the whole
    # inner box), both orders of query / box
    outer = kitti_labels(rng, 400, dims=((4.0, 6.0), (3.0, 4.0)))
    r_in = 0.5 * outer[:, 3]
    inner = np.zeros_like(outer)
    hd = r_in * rng.uniform(0.3, 0.9, 400)                 # inner half diagonal
    ia = rng.uniform(0.2, 1.3, 400)
    inner[:, 2], inner[:, 3] = 2 * hd * np.cos(np.arctan(1 / ia)), 2 * hd * np.sin(np.arctan(1 / ia))
    off = (r_in - hd) * rng.uniform(0, 0.95, 400)
    oa = rng.uniform(-math.pi, math.pi, 400)
    inner[:, 0], inner[:, 1] = outer[:, 0] + off * np.cos(oa), outer[:, 1] + off * np.sin(oa)
    inner[:, 4] = rng.uniform(-math.pi, math.pi, 400)
    add("nested", outer[:200], inner[:200])
    add("nested", inner[200:], outer[200:])

    # exact axis-aligned integer configurations (angle 0: cos 1, sin 0 exactly; all corners and areas exact in float32)
    ex_q, ex_b, ex_v = [], [], []

    def exact(q, b, inter):
        aq, ab = q[2] * q[3], b[2] * b[3]
        ex_q.append(q); ex_b.append(b)
        ex_v.append([inter / (aq + ab - inter), inter / aq, inter / ab, inter])
    for _ in range(250):
        w, h = (int(v) * 4 for v in rng.integers(1, 4, 2))
        x0, y0 = (int(v) * 2 for v in rng.integers(-20, 20, 2))
        sx = int(rng.integers(0, 2)) * 2 - 1
        big = [x0, y0, w, h, 0.0]
        exact(big, [x0 + sx * w, y0, w, h, 0.0], 0.0)                                      # shared edge
        exact(big, [x0 + sx * w, y0 + h, w, h, 0.0], 0.0)                                  # touching corner
        exact(big, [x0 + sx * w // 2, y0, w, h, 0.0], w * h / 2)                           # half overlap
        exact(big, [x0, y0, w // 2, h // 2, 0.0], w * h / 4)                               # containment, centred
        ix = x0 - w // 2 + w // 4                                                           # nested, shared edge
        exact(big, [ix, y0, w // 2, h // 2, 0.0], w * h / 4)
    order = rng.permutation(len(ex_q))
    ex_q, ex_b, ex_v = np.array(ex_q)[order], np.array(ex_b)[order], np.array(ex_v)[order]
    swap = rng.uniform(size=len(ex_q)) < 0.5                # query and box exchanged: criteria 0 and 1 swap
    ex_q[swap], ex_b[swap] = ex_b[swap].copy(), ex_q[swap].copy()
    ex_v[swap] = ex_v[swap][:, [0, 2, 1, 3]]
    add("exact_aa", ex_q, ex_b, ex_v)

    # near copies, perturbed by 1e-6 ... 1e-3 in every parameter
    lab = kitti_labels(rng, 1200)
    eps = 10.0 ** rng.uniform(-6, -3, (1200, 1))
    add("near_copy", lab + eps * rng.normal(0, 1, (1200, 5)), lab)
    # turned copies: by pi, by pi / 2 with the dims swapped, by 2 pi; exact copies
    lab = kitti_labels(rng, 600)
    t = lab.copy(); t[:200, 4] += math.pi
    t[200:400, 4] += math.pi / 2; t[200:400, 2], t[200:400, 3] = lab[200:400, 3], lab[200:400, 2]
    t[400:, 4] += 2 * math.pi
    add("turned_copy", t, lab)
    lab = np.concatenate([kitti_labels(rng, 150), random_rboxes(rng, 50)])
    add("exact_copy", lab, lab)

    # small pedestrians far away
    lab = kitti_labels(rng, 800, dims=PED, z=(60.0, 80.0))
    add("far_pedestrian", detections(rng, lab, rng.choice([0.15, 0.3, 0.55], 800)), lab)

    # headings up to +-4 pi
    lab = kitti_labels(rng, 800)
    det = detections(rng, lab, rng.choice([0.15, 0.3, 0.55], 800))
    lab[:, 4] = rng.uniform(-4 * math.pi, 4 * math.pi, 800)
    det[:, 4] = lab[:, 4] + rng.normal(0, 0.2, 800) + 2 * math.pi * rng.integers(-1, 2, 800)
    add("wide_angle", det, lab)

    # DontCare rows: location -1000, dims -1, rotation_y -10 -> BEV (-1000, -1000, -1, -1, -10)
    dc = np.tile([-1000.0, -1000.0, -1.0, -1.0, -10.0], (300, 1))
    lab = kitti_labels(rng, 300)
    add("dontcare", dc[:150], lab[:150])
    add("dontcare", lab[150:], dc[150:])
    near = dc[:50] + np.concatenate([rng.uniform(-1, 1, (50, 2)), np.zeros((50, 3))], 1)
    add("dontcare", near, dc[:50])                          # DontCare against (nearly) DontCare

    # zero-area boxes: a zero dim on one side, the other, or both
    lab = kitti_labels(rng, 300)
    z = lab.copy()
    z[:, 0] += rng.normal(0, 0.3, 300); z[:, 1] += rng.normal(0, 0.3, 300)
    z[:100, 2] = 0.0; z[100:200, 3] = 0.0; z[200:, 2:4] = 0.0
    add("zero_area", z[:150], lab[:150])
    add("zero_area", lab[150:250], z[150:250])
    add("zero_area", z[250:], z[250:] + np.array([0.2, 0.1, 0, 0, 0.3]))
    return (np.concatenate(Q).astype(np.float32), np.concatenate(B).astype(np.float32), np.concatenate(C).astype(np.int8),
            np.concatenate(X))


def evaluate_catalogue(q, b):
    M = len(q)
    r32, r64, w32 = np.zeros((M, 4), np.float32), np.zeros((M, 4)), np.zeros((M, 4), np.float32)
    over32, over64 = np.zeros(M, bool), np.zeros(M, bool)
    n32, n64 = np.zeros(M, np.int8), np.zeros(M, np.int8)
    for i in range(M):
        for c, crit in enumerate(CRITERIA):
            v, o = ref_pair(q[i], b[i], crit, np.float32)
            r32[i, c], over32[i] = v, over32[i] or o
            v, o = ref_pair(q[i], b[i], crit, np.float64)
            r64[i, c], over64[i] = v, over64[i] or o
        w32[i] = [ref_pair_wide(q[i], b[i], crit) for crit in CRITERIA] if over32[i] else r32[i]
        n32[i], n64[i] = candidates(q[i], b[i], np.float32), candidates(q[i], b[i], np.float64)
    return r32, r64, w32, over32, over64, n32, n64


STABLE_ABS, STABLE_REL = 2e-5, 2e-5


TIE_CLASSES = ("exact_copy", "turned_copy")       # every vertex test is an exact tie: agreement there is coincidence


def stable_mask(r32, r64, over32, over64, n32, n64, cls):
    """the pairs on which the reference's own answer does not depend on round-off"""
    with np.errstate(all="ignore"):
        d = np.abs(r32.astype(np.float64) - r64)
        ok = (~over32 & ~over64 & (n32 == n64) & np.isfinite(r32).all(1) & np.isfinite(r64).all(1)
              & (d[:, :3] <= STABLE_ABS).all(1) & (d[:, 3] <= STABLE_REL * np.maximum(np.abs(r64[:, 3]), 1.0)))
    return ok & ~np.isin(cls, [CLASSES.index(c) for c in TIE_CLASSES])


# ------------------------------------------------------------------------------------------------ kernel / wrapper runs
def kernel_matrices(rng):
    """the reference's host wrapper -> emulated rotate_iou_kernel_eval on 70 x 131 (partial tiles both ways), float32;
    checked against per-pair devRotateIoUEval(query, box)"""
    boxes = np.concatenate([random_rboxes(rng, 40), kitti_labels(rng, 30) * [0.1, 0.1, 1, 1, 1] + [0, 15, 0, 0, 0]]).astype(np.float32)
    qboxes = np.concatenate([random_rboxes(rng, 90), detections(rng, boxes[40:].astype(np.float64), 0.3)[:30],
                             boxes[:11].astype(np.float64) + rng.normal(0, 0.05, (11, 5))]).astype(np.float32)
    sample = np.sort(rng.choice(70 * 131, 1500, replace=False))
    out = {"mat.boxes": boxes, "mat.qboxes": qboxes, "mat.sample": sample}
    for crit in CRITERIA:
        STATE.dt = np.float32
        with np.errstate(all="ignore"):
            m = RR.rotate_iou_gpu_eval(boxes, qboxes, crit)
        assert m.shape == (70, 131) and m.dtype == np.float32
        per = np.array([[ref_pair(qboxes[k], boxes[n], crit, np.float32)[0] for k in range(131)] for n in range(70)], np.float32)
        assert np.array_equal(m, per), "emulated kernel != per-pair devRotateIoUEval(query, box)"
        out["mat.ref32.c%d" % crit] = m
        out["mat.pair32.c%d" % crit] = per.reshape(-1)[sample]           # the per-pair calls, a fixed sample of them
        out["mat.ref64.c%d" % crit] = np.array([[ref_pair(qboxes[k], boxes[n], crit, np.float64)[0] for k in range(131)]
                                                for n in range(70)])
    return out


def boxes3d(rng, n, dims=None):
    lab = kitti_labels(rng, n, dims)
    y = rng.uniform(1.0, 2.5, n)
    h = rng.uniform(1.2, 2.2, n)
    return np.stack([lab[:, 0], y, lab[:, 1], lab[:, 2], h, lab[:, 3], lab[:, 4]], 1)


def golden_3d(rng):
    """d3_box_overlap (emulated rotate_iou_gpu_eval, criterion 2, then d3_box_overlap_kernel) for criteria -1 / 0 / 1"""
    a = boxes3d(rng, 48)
    a[40:] = [-1000.0, -1000.0, -1000.0, -1.0, -1.0, -1.0, -10.0]            # DontCare rows
    det = detections(rng, a[:40][:, [0, 2, 3, 5, 6]], rng.choice([0.15, 0.3, 0.55], 40))
    b = np.repeat(a[:40], 2, axis=0)
    b[:40][:, [0, 2, 3, 5, 6]] = det
    b[:40, 1] += rng.normal(0, 0.15, 40)                                   # generic: heights overlap partly
    b[40:60, 1] = a[:20, 1] - a[:20, 4]                                    # touching heights: iw = 0 exactly
    b[40:60, 4] = rng.uniform(1.2, 2.2, 20)
    b[60:70, 1] = a[20:30, 1] - a[20:30, 4] - rng.uniform(0.1, 1.0, 10)     # one box above the other
    b[70:80, 1] = a[30:40, 1] + 0.5 * a[30:40, 4]                          # half the height shared
    b = np.concatenate([b, a[40:44]])                                      # DontCare against DontCare
    out = {"d3.boxes": b, "d3.qboxes": a}
    for crit in (-1, 0, 1):
        STATE.dt = np.float32
        with np.errstate(all="ignore"):
            r = RE.d3_box_overlap(b, a, crit)
        out["d3.ref32.c%d" % crit] = r
    # stability of each pair's bird's-eye-view intersection, as for the catalogue (criterion 2 only)
    bq, bb = a[:, [0, 2, 3, 5, 6]].astype(np.float32), b[:, [0, 2, 3, 5, 6]].astype(np.float32)
    st = np.zeros((len(b), len(a)), bool)
    for n in range(len(b)):
        for k in range(len(a)):
            v32, o32 = ref_pair(bq[k], bb[n], 2, np.float32)
            v64, o64 = ref_pair(bq[k], bb[n], 2, np.float64)
            st[n, k] = (not o32 and not o64 and candidates(bq[k], bb[n], np.float32) == candidates(bq[k], bb[n], np.float64)
                        and abs(v32 - v64) <= STABLE_REL * max(abs(v64), 1.0))
    out["d3.bev_stable"] = st
    return out


def golden_end_to_end():
    gts, dts = synth.random_kitti_annos(5, frames=12)
    STATE.dt = np.float32
    with np.errstate(all="ignore"):
        text, res = RE.kitti_eval(gts, dts, ["Pedestrian", "Cyclist", "Car"], eval_types=["bbox", "bev", "3d"])
    return {"e2e.keys": np.asarray(list(res.keys())), "e2e.values": np.asarray([float(res[k]) for k in res], np.float64),
            "e2e.text": np.frombuffer(text.encode(), dtype=np.uint8)}


def main():
    rng = np.random.default_rng(20261016)
    q, b, cls, exact = catalogue(rng)
    r32, r64, w32, over32, over64, n32, n64 = evaluate_catalogue(q, b)
    stable = stable_mask(r32, r64, over32, over64, n32, n64, cls)
    # self-consistency before anything is written
    ex = ~np.isnan(exact[:, 0])
    with np.errstate(all="ignore"):
        assert np.array_equal(r32[ex], exact[ex].astype(np.float32), equal_nan=True), "closed forms"
    assert (r32[cls == CLASSES.index("disjoint")] == 0).all() and (r64[cls == CLASSES.index("disjoint")] == 0).all()
    assert n32.max() <= 16 and n64.max() <= 16
    out = {"q": q, "b": b, "cls": cls, "exact": exact, "ref32": r32, "ref64": r64, "wide32": w32, "overrun32": over32,
           "overrun64": over64, "ncand32": n32, "ncand64": n64, "stable": stable, "classes": np.asarray(CLASSES)}
    out.update(kernel_matrices(rng))
    out.update(golden_3d(rng))
    out.update(golden_end_to_end())
    F4.save("rotate_iou_ref.npz", **out)

    per_class = {}
    for c, name in enumerate(CLASSES):
        m = cls == c
        per_class[name] = {"pairs": int(m.sum()), "stable": int((m & stable).sum()), "overrun32": int((m & over32).sum()),
                           "max_candidates": int(max(n32[m].max(), n64[m].max()))}
    meta = {"numpy": np.__version__, "generator": "tests/golden/make_rotate_iou_golden.py",
            "reference_modules_run": [RR.__file__, RE_ROT.__file__, RE.__file__],
            "executed": ["rotate_iou_kernel_eval (emulated launch, float32)", "rotate_iou_gpu_eval", "devRotateIoUEval",
                         "inter", "quadrilateral_intersection", "rbbox_to_corners", "point_in_quadrilateral",
                         "line_segment_intersection", "sort_vertex_in_convex_polygon", "area", "trangle_area",
                         "bev_box_overlap", "d3_box_overlap", "d3_box_overlap_kernel", "kitti_eval"],
            "shim": SHIM, "numpy2_vs_numba_typing": NUMPY2_TYPING,
            "stable": {"abs_iou": STABLE_ABS, "rel_area": STABLE_REL,
                       "rule": "no overrun at either precision, equal candidate counts, |ref32 - ref64| within the bounds "
                               "for all four criteria, not a copy class (%s)" % ", ".join(TIE_CLASSES)},
            "pairs": int(len(q)), "max_candidates": int(max(n32.max(), n64.max())), "per_class": per_class}
    with open(os.path.join(HERE, "meta_rotate_iou.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps(per_class, indent=1))


if __name__ == "__main__":
    main()
