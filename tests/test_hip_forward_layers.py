"""The train plan's forward of backbone + neck, layer by layer against fp64 on the plan's own maps, statistics included.

One train-mode forward per (config, shape) with MONOCON_HIP_PLAN_DEBUG=1.  Every node is read with `mc_train_debug_node`
(which = 0: a lazy node is formed with the plan's own coefficients), the running buffers are the model's bound tensors, and
`plan_graph.forward_reference` forms every forward quantity of every layer in float64 from the buffers AROUND that layer:
nothing flips, nothing is amplified.  The tests are per quantity class, so a failure names its kernel family:

    conv nodes        the conv kernel, bn_finalize's coefficients, affine_act or the lazy formation (stem, 3x3s1, 3x3s2, 1x1)
    batch statistics  chan_reduce / the conv epilogues' (sum, sum of squares) partials, partial_fold, bn_finalize
    running buffers   bn_finalize's update: momentum, n / (n - 1), the in-place read-then-write of running_mean (which is
                      also the shift of the variance sums), num_batches_tracked; the two dead outer `project` BatchNorms too
    pool nodes        maxpool2 on a stored and on a lazy input
    deconv nodes      deconv4 on a stored and on a lazy input

Tolerances -- no number is fitted to the code under test (U = 2^-24, m = 0.1):

  conv nodes, deconv nodes: elementwise |got - ref| / M, M the same operation on absolute values in fp64
    (|a| conv2d(|x|, |w|) + |b| + |res|), floored at 2^-10 of its tensor maximum.  Yard-stick: the same node by torch in
    float32 from the same float32 buffers (F.conv2d, F.batch_norm(training=True)), worst per kind.  Gate: HIP <= 5 x worst
    + 4 U (the 5 and the 4 U are test_gradients_match_reference's), in f16x2 plus the operand-split term 2^-21 T_c |a_c| / M
    (T_c = sum over the sources of max |x_s| sum |w_c,s|, test_hip_operand_scale), plus the statistic bounds below carried
    through the affine: |a_c| (|y - mean| b_var / (2 (var + eps)) + b_mean).
  batch statistics, recovered from the running buffers: mean_gpu = (rm' - (1 - m) rm) / m, likewise the variance (times
    (n - 1) / n: the biased one).  The recovery's own fp32 rounding, 4 U (|rm'| + |rm|) / m, is part of the bound.
      b_mean = (L + 8) U E|y - shift| + dy_c
      b_var  = (L + 8) U E[(y - shift)^2] + 2 |m0| b_mean + 2 E|y - shift| dy_c            (m0 = mean - shift)
    L, the longest single fp32 chain before the double fold (bn_finalize's float build adds its partials in double too: each
    thread's `s1 += p[0]` has a double accumulator), per producer as the plan's `[plan] forward` lines name it:
      fp32, fp32_ws, split, wres    the tilings' epilogue: 16 accumulators per lane and one shuffle of a 4x8 patch   L = 32
      row, row_lazy, thin16         one partial per output row                                                   L = W_out
      stem_f16                      the fp16-pipe stem, one partial per output row                               L = W_out
      chan_reduce                   <= 256 rows / RG per thread + RG row groups (the stem in fp32 / bf16x3)        L = 257
    dy_c = 4 sqrt(K) U max M_y,c (a K-term fp32 accumulation as a random walk with a factor 4; + 2^-21 T_c in f16x2): the
    backward-layers model of how far the GPU's own y lies from the reference's.
  running buffers directly: 4 U x their magnitude sum (1 - m) |old| + m |statistic|, + m b_mean, resp. + m b_var n / (n - 1);
    num_batches_tracked exact.
  pool nodes: bit-equal to max_pool2d of the input node as read; where the input is lazy (the pool forms z itself and may
    round the fma differently from the debug read): within 4 U of the max-pooled |a| |y64| + |b|.

Config S is the SECOND forward of one model (the first ran on the stressed batch with the image times 64): a stale amax slot
from step 1 costs 6 of the split's 22 bits, a stale partial row moves the statistics, and the shift has moved under the sums.

Measured (MI355X): see MEASURED below and DESIGN.md 3c ("The train forward, layer by layer").
"""
import copy
import math
import re
import time

import pytest
import torch

from plan_graph import (BN_MOMENTUM, EPS, STEM, _bn_of, _model, _node_dims, _plan_convs, _read_node, forward_reference,
                        plan_graph, stderr_lines, stressed_batch, stressed_state_dict)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LAZY_D = {"MONOCON_HIP_LAZY_Z": "3", "MONOCON_HIP_LAZY_MIN": "0"}
CONFIGS = {   # precision, state, switches
    "A": ("fp32", "golden", {}),
    "B": ("bf16x3", "golden", {}),
    "C": ("f16x2", "golden", {"MONOCON_HIP_LAZY_Z": "0"}),
    "D": ("f16x2", "stressed", dict(LAZY_D)),
    "E": ("f16x2", "stressed", dict(LAZY_D, MONOCON_HIP_LAZY_FEAT="1")),
    "Z32": ("fp32", "fresh", {}),        # golden weights, every running_mean 0 and running_var 1: the shift far from the mean
    "Z16": ("f16x2", "fresh", {}),
    "S": ("f16x2", "stressed", dict(LAZY_D)),      # the second forward of one model
}
SHAPES = {
    "3x96x160": (3, 96, 160),       # odd batch, 3x5 maps at level5 (n = 45), patch counts not a multiple of 4
    "2x64x224": (2, 64, 224),       # a half-filled last strip of the 16-column kernels, 2x7 maps (n = 28)
    "2x96x1248": (2, 96, 1248),     # KITTI's width, the odd-tile paths (config D only)
    # partial_fold + bn_finalize<double> start at 2048 partial rows.  The full-resolution layers leave one row of partials per
    # OUTPUT ROW (stem_f16, thin16, the fp32 row kernel: B * H rows) and chan_reduce fewer than 2048 blocks below 2^19
    # pixels, so 2x96x1248 stays on the float build everywhere (192 and 1872 rows; its 7488 patches would be a tiling's);
    # B * H = 2048 on narrow frames reaches the double build at fewer pixels than 1248 has (configs A and D)
    "8x256x96": (8, 256, 96),
}
CASES = ([(c, s) for c in "ABCDE" for s in ("3x96x160", "2x64x224")] + [("D", "2x96x1248"), ("A", "8x256x96"), ("D", "8x256x96")] +
         [(c, "3x96x160") for c in ("Z32", "Z16", "S")])
CASE_IDS = ["%s-%s" % cs for cs in CASES]
SWITCHES = ("LAZY_Z", "LAZY_MIN", "LAZY_FEAT", "ZBITS", "GRAD_POOL", "STEM_FUSE", "BM_EPILOGUE", "WRES_BWD", "DUAL_STREAM")
PATCH_PRODUCERS = ("fp32", "fp32_ws", "split", "wres")
ROW_PRODUCERS = ("row", "row_lazy", "thin16", "stem_f16")
FOLD_MIN_NB = 2048          # kernels_train.hip: from this many partial rows on partial_fold + bn_finalize<double>
CONV_KINDS = ("stem", "3x3s1", "3x3s2", "1x1")
# measured on an MI355X.  Conv kinds, deconv: worst HIP error / float32 yard-stick error (gate: 5 x + 4 U, + the terms of the
# module docstring); statistics and running buffers: worst measured / bound (gate: 1)
MEASURED = """
config       stem   3x3s1  3x3s2  1x1    deconv | batch mean  batch var  running_mean  running_var | worst E[(y - shift)^2] / var
A fp32       0.95   1.45   1.10   1.19   1.00   | 0.077       0.032      0.10          0.034       | 2.07
B bf16x3     0.95   1.00   0.92   0.55   1.00   | 0.080       0.028      0.10          0.031       | 2.07
C f16x2      0.49   0.67   1.01   0.58   1.00   | 0.052       0.016      0.060         0.016       | 2.07
D stressed   0.64   0.61   1.36   1.80   1.00   | 0.020       0.028      0.021         0.030       | 443 (level3.project.0)
E stressed   0.63   0.61   1.00   1.80   1.00   | 0.020       0.016      0.021         0.017       | 273
Z fp32       0.84   1.17   1.00   1.24   1.00   | 0.0082      0.017      0.0082        0.018       | 33.5 (level5.project.0)
Z f16x2      0.39   0.64   1.00   0.89   1.00   | 0.0076      0.0097     0.0076        0.010       | 33.5
S 2nd step   0.62   0.55   0.92   0.73   1.00   | 0.029       0.099      0.031         0.17        | 195 (level5.root.conv)
(worst over the config's shapes; A includes 8x256x96, D 2x96x1248 and 8x256x96.  The float32 yard-stick itself: 1.2e-7 ..
3.8e-7 of the magnitude sum.  With the split term and the statistic bounds the worst conv node uses 0.06 of its whole gate;
none needs them: the worst, 1.80 x float32, passes the plain 5 x + 4 U.  Statistics by producer, measured / bound:
chan_reduce 0.009 .. 0.011, fp32 0.017 .. 0.077, fp32_ws 0.012 .. 0.067, split 0.009 .. 0.080, row 0.003 .. 0.026,
row_lazy 0.002 .. 0.003, thin16 0.001 .. 0.007, stem_f16 0.007 .. 0.099 (S; 0.028 on the double build at 8x256x96); no plan of
the matrix chose wres for a forward layer.  Lazy pools: bit-equal to the debug read everywhere (0 of 4 U).  running_var
beside torch's float32 update of the same buffers, error / magnitude sum: Z 2.9e-7 against 1.4e-7 -- the shift at 0 costs a
fresh network nothing measurable; D 8.1e-6 against 5.2e-7, S 3.2e-6 against 3.1e-7 -- E[(y - shift)^2] / var of some hundred
costs the stressed state a factor 10 .. 16, inside the bound (0.03 .. 0.17 of it).  Per case: model, plan and forward 0.2 ..
0.4 s, reference and bounds 0.2 .. 1.3 s on the host.)
"""


def _say(line):
    print("\n[forward layers] " + line)


class Step:
    pass


def fresh_state_dict(sd):
    """the state with every backbone / neck BatchNorm as a new network has it: running_mean 0, running_var 1"""
    out = {k: v.clone() for k, v in sd.items()}
    for _, bn in _plan_convs():
        out[bn + ".running_mean"].zero_()
        out[bn + ".running_var"].fill_(1.0)
    return out


def _chain_length(producer, Wout):
    """L of the module docstring; a producer that is not listed there has no bound: KeyError"""
    if producer in PATCH_PRODUCERS:
        return 32
    if producer in ROW_PRODUCERS:
        return Wout
    return {"chan_reduce": 257}[producer]


def parse_forward_lines(log):
    """{bn: (node or -1, producer, partial rows, 'float' / 'double', 'lazy' / 'stored' / 'dead')} and the nodes that were lazy
    but stored after all, from the plan's debug lines"""
    prod, materialised = {}, set()
    for l in log:
        mm = re.match(r"\[plan\] forward (\S+)\s+node\s+(-?\d+)\s+statistics by (\S+)\s+(\d+) partial rows\s+finalize (\S+)\s+z (\S+)", l)
        if mm:
            prod[mm.group(1)] = (int(mm.group(2)), mm.group(3), int(mm.group(4)), mm.group(5), mm.group(6))
        mm = re.search(r"lazy node (\d+) .* materialised", l)
        if mm:
            materialised.add(int(mm.group(1)))
    return prod, materialised


def _run_step(cfg, shape, golden_sd, monkeypatch):
    """the forward of (config, shape), its nodes and running buffers, the plan's debug lines and the fp64 reference"""
    precision, state, env = CONFIGS[cfg]
    B, H, W = SHAPES[shape]
    for k in SWITCHES:
        monkeypatch.delenv("MONOCON_HIP_" + k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                       # read when the train plan is built: a fresh model per step
    monkeypatch.setenv("MONOCON_HIP_PLAN_DEBUG", "1")
    stressed = state == "stressed"
    sd = {"golden": lambda: golden_sd, "stressed": lambda: stressed_state_dict(golden_sd),
          "fresh": lambda: fresh_state_dict(golden_sd)}[state]()
    from hipmonocon import synth
    batch = stressed_batch(6300 + W, B, H, W) if stressed else synth.make_batch(6300 + W, B, H, W)

    def forward(m, img):
        gb = {"img": img.cuda(), "label": {k: v.cuda() for k, v in batch["label"].items()}, "img_metas": batch["img_metas"]}
        m(gb)
        torch.cuda.synchronize()

    t0 = time.time()
    with stderr_lines() as err:
        m = _model(sd, precision)
        if cfg == "S":
            forward(m, batch["img"] * 64.0)
        sd_before = copy.deepcopy({k: v.detach().cpu() for k, v in m.state_dict().items()})
        forward(m, batch["img"])
    S = Step()
    S.cfg, S.shape, S.precision, S.dims_in = cfg, shape, precision, (B, H, W)
    S.graph = G = plan_graph()
    S.node_dims = [_node_dims(m, i) for i in range(G.n_nodes)]
    S.act = {i: _read_node(m, i) for i in range(G.n_nodes)}
    S.sd_before = sd_before
    S.sd_after = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    del m
    torch.cuda.empty_cache()
    S.gpu_seconds = time.time() - t0
    S.log = [l for l in err if l.startswith("[plan]")]
    S.producer, S.materialised = parse_forward_lines(S.log)
    t0 = time.time()
    S.img = batch["img"]
    S.R = forward_reference(G, S.act, S.img, sd_before, yardstick=True)
    _evaluate(S)
    S.host_seconds = time.time() - t0
    S.act = S.R = S.img = S.sd_before = S.sd_after = None           # (only the figures are kept)
    _say("%s %s: model, plan and forward %.1f s, reference + bounds %.1f s on the host" % (cfg, shape, S.gpu_seconds, S.host_seconds))
    return S


def _evaluate(S):
    """every compared quantity of the forward as (measured, allowed) figures:
    S.conv[kind] = [(layer, hip error, float32 error, worst |got - ref| / allowed)] for the conv kinds and "deconv";
    S.ratio[class] = [(label, measured / bound)] for the statistics classes and "lazy pools"; S.bad_pools, S.bad_nbt: lines;
    S.run_err[buffer] = [(HIP error / magnitude sum, the float32 yard-stick's, BatchNorm)];
    S.shift_cost = {conv: max over channels of E[(y - shift)^2] / var}; S.b_mean, S.b_var = {conv: the statistic bounds per
    channel}, S.tol = {(class, BatchNorm): the whole allowance of a statistics class per channel}; S.checked: what the
    coverage test counts"""
    G, R, act = S.graph, S.R, S.act
    m = BN_MOMENTUM
    f16 = S.precision == "f16x2"
    dims = G.dims(*S.dims_in)
    v = lambda t: t[None, :, None, None]          # noqa: E731
    S.conv, S.ratio, S.yard, S.gate, S.bad_pools, S.bad_nbt, S.shift_cost = {}, {}, {}, {}, [], [], {}
    S.nbt, S.run_err = {}, {"running_mean": [], "running_var": []}
    S.checked = {"finalize": set(), "consumers": set(), "nodes": set(), "bns": set()}

    S.tol = {}

    def ratios(cls, label, err, tol, bn=None):
        S.ratio.setdefault(cls, []).append((label, float((err / tol.clamp_min(1e-300)).max())))
        if bn is not None:
            S.tol[(cls, bn)] = tol

    # ---- statistics and running buffers, every BatchNorm of the plan (dead projects included)
    S.b_mean, S.b_var = b_mean, b_var = {}, {}
    for name, bn in _plan_convs():
        st = R.stats[name]
        node, prod, nb, fin, zstate = S.producer[bn]
        n = st["n"]
        Wout = S.dims_in[2] if name == STEM else (dims[st["node"]][3] if st["node"] is not None else
                                                   dims[dict(G.dead)[name]][3])
        L = _chain_length(prod, Wout)
        dy_c = 4 * math.sqrt(st["K"]) * U * st["ymag_max"]
        if f16:
            dy_c = dy_c + 2.0 ** -21 * st["tmax"]
        bm = (L + 8) * U * st["e1"] + dy_c
        bv = (L + 8) * U * st["e2"] + 2 * st["m0"].abs() * bm + 2 * st["e1"] * dy_c
        b_mean[name], b_var[name] = bm, bv
        rm0, rv0 = S.sd_before[bn + ".running_mean"].double(), S.sd_before[bn + ".running_var"].double()
        rm1, rv1 = S.sd_after[bn + ".running_mean"].double(), S.sd_after[bn + ".running_var"].double()
        label = "%s (%s, %s)" % (bn, prod, fin)
        ratios("batch mean", label, ((rm1 - (1 - m) * rm0) / m - st["mean"]).abs(), bm + 4 * U * (rm1.abs() + rm0.abs()) / m, bn)
        shrink = (n - 1.0) / n
        ratios("batch var", label, ((rv1 - (1 - m) * rv0) / m * shrink - st["var"]).abs(),
               bv + 4 * U * (rv1.abs() + rv0.abs()) / m * shrink, bn)
        run = R.running[bn]
        ratios("running_mean", label, (rm1 - run["rm"].ref).abs(), 4 * U * run["rm"].mag + m * bm, bn)
        ratios("running_var", label, (rv1 - run["rv"].ref).abs(), 4 * U * run["rv"].mag + m * bv / shrink, bn)
        for key, t, got in (("running_mean", run["rm"], rm1), ("running_var", run["rv"], rv1)):      # beside torch's float32 update
            mag = t.mag.clamp_min(1e-300)
            S.run_err[key].append((float(((got - t.ref).abs() / mag).max()), float(((t.f32.double() - t.ref).abs() / mag).max()), bn))
        got_nbt = int(S.sd_after[bn + ".num_batches_tracked"])
        S.nbt[bn] = got_nbt
        if got_nbt != run["nbt"]:
            S.bad_nbt.append("%s.num_batches_tracked is %d, expected %d" % (bn, got_nbt, run["nbt"]))
        S.shift_cost[name] = float((st["e2"] / st["var"].clamp_min(1e-300)).max())
        S.checked["finalize"].add(fin)
        S.checked["bns"].add(bn)
        assert fin == ("double" if nb >= FOLD_MIN_NB else "float"), (bn, nb, fin)

    # ---- which nodes the plan holds lazy when their consumers read them
    lazy = {node for node, prod, nb, fin, zstate in S.producer.values() if zstate == "lazy"} - S.materialised
    S.lazy = lazy

    # ---- conv nodes
    for kind in CONV_KINDS:
        rows = [r for r in R.layers if r[0] == kind]
        S.yard[kind] = max(t.f32_err() for _, _, _, t in rows)
        S.gate[kind] = 5 * S.yard[kind] + 4 * U
        for _, name, o, t in rows:
            st = R.stats[name]
            got = act[o]
            assert got.shape == t.ref.shape, (name, got.shape, t.ref.shape)
            e = (got.double() - t.ref).abs()
            Mf = t.floored()
            a = st["a"].abs()
            allowed = S.gate[kind] * Mf + v(a) * (st["dev"] * v(b_var[name] / (2 * (st["var"] + EPS))) + v(b_mean[name]))
            if f16:
                allowed = allowed + v(2.0 ** -21 * st["tmax"] * a)
            S.conv.setdefault(kind, []).append((name, float((e / Mf).max()), t.f32_err(), float((e / allowed).max())))
            S.checked["nodes"].add(o)
            srcs = [] if name == STEM else next(r[1] for r in G.recs if r[0] == name)
            S.checked["consumers"] |= {("conv", "lazy" if s in lazy else "stored") for s in srcs}
    # ---- deconv nodes
    S.yard["deconv"] = max(t.f32_err() for _, _, _, t in R.deconvs)
    S.gate["deconv"] = 5 * S.yard["deconv"] + 4 * U
    for name, i, o, t in R.deconvs:
        e = (act[o].double() - t.ref).abs() / t.floored()
        S.conv.setdefault("deconv", []).append((name, float(e.max()), t.f32_err(), float(e.max()) / S.gate["deconv"]))
        S.checked["nodes"].add(o)
        S.checked["consumers"].add(("deconv", "lazy" if i in lazy else "stored"))
    # ---- pool nodes
    zmag_of = {st["node"]: st["zmag"] for st in R.stats.values() if st["node"] is not None}
    for i, o, want in R.pools:
        if i in lazy:          # (a lazy map has no residual: |a| |y64| + |b| is the size of what the pool forms)
            ratios("lazy pools", "pool node %d of lazy node %d" % (o, i), (act[o].double() - want.double()).abs(),
                   4 * U * torch.nn.functional.max_pool2d(zmag_of[i], 2, 2))
        elif not torch.equal(act[o], want):
            S.bad_pools.append("pool node %d of node %d is not bit-equal" % (o, i))
        S.checked["nodes"].add(o)
        S.checked["consumers"].add(("pool", "lazy" if i in lazy else "stored"))


_DONE = {}


@pytest.fixture(scope="module", params=CASES, ids=CASE_IDS)
def step(request, golden_sd):
    """one forward and one run of the reference per (config, shape); the tests below only read its figures"""
    with pytest.MonkeyPatch.context() as mp:
        _DONE[request.param] = _run_step(request.param[0], request.param[1], golden_sd, mp)
    return _DONE[request.param]


def _report(S, cls):
    rows = S.ratio.get(cls, [])
    if not rows:
        return []
    worst = max(rows, key=lambda r: r[1])
    _say("%s %s %-14s worst measured / bound %.3g (%s)" % (S.cfg, S.shape, cls, worst[1], worst[0]))
    return ["%s %s: %.3g of the bound" % (cls, r[0], r[1]) for r in rows if not r[1] <= 1.0]


def _report_conv(S, kinds):
    bad = []
    for kind in kinds:
        rows = S.conv[kind]
        worst = max(rows, key=lambda r: r[1])
        _say("%s %s %-8s HIP %.3g / float32 %.3g = %.2f (%s); worst of the gate %.3g"
             % (S.cfg, S.shape, kind, worst[1], S.yard[kind], worst[1] / max(S.yard[kind], 1e-30), worst[0], max(r[3] for r in rows)))
        bad += ["%s %s: %.3g of the gate (error %.3g, float32 %.3g)" % (kind, r[0], r[3], r[1], r[2]) for r in rows if not r[3] <= 1.0]
    return bad


# ------------------------------------------------------------------------------------------------ the graph
def test_node_dims_and_plan_lines(step):
    """every node's (B, C, H, W) equals the graph's; the plan names a statistics producer for every BatchNorm of the plan,
    the dead projects included, and at the node the graph gives the layer"""
    S = step
    G = S.graph
    assert S.node_dims == G.dims(*S.dims_in)
    assert set(S.producer) == {bn for _, bn in _plan_convs()}
    want = {_bn_of(STEM): 0}
    want.update({_bn_of(r[0]): r[4] for r in G.recs})
    want.update({_bn_of(name): -1 for name, _ in G.dead})
    assert {bn: p[0] for bn, p in S.producer.items()} == want
    assert {bn for bn, p in S.producer.items() if p[4] == "dead"} == {_bn_of(name) for name, _ in G.dead}


# ------------------------------------------------------------------------------------------------ the quantity classes
def test_conv_nodes(step):
    bad = _report_conv(step, CONV_KINDS)
    assert not bad, "\n".join(bad)


def test_batch_statistics(step):
    S = step
    bad = _report(S, "batch mean") + _report(S, "batch var")
    for p in sorted({q[1] for q in S.producer.values()}):
        rows = [r for c in ("batch mean", "batch var") for r in S.ratio[c] if "(%s," % p in r[0]]
        _say("%s %s   statistics left by %-11s %3d figures, worst measured / bound %.3g" % (S.cfg, S.shape, p, len(rows), max(r[1] for r in rows)))
    if S.cfg.startswith("Z"):
        _say("%s %s   E[(y - shift)^2] / var per layer: " % (S.cfg, S.shape) +
             ", ".join("%s %.3g" % (n.replace("backbone.", "").replace("neck.", ""), c) for n, c in S.shift_cost.items()))
    worst = max(S.shift_cost, key=S.shift_cost.get)
    _say("%s %s   worst E[(y - shift)^2] / var %.3g (%s)" % (S.cfg, S.shape, S.shift_cost[worst], worst))
    assert not bad, "\n".join(bad)


def test_running_buffers(step):
    S = step
    bad = _report(S, "running_mean") + _report(S, "running_var") + S.bad_nbt
    assert S.checked["bns"] == {bn for _, bn in _plan_convs()}
    for key, rows in S.run_err.items():
        h = max(rows)
        _say("%s %s %-14s error / magnitude sum: HIP %.3g (%s), float32 there %.3g, float32 worst %.3g"
             % (S.cfg, S.shape, key, h[0], h[2], h[1], max(r[1] for r in rows)))
    assert set(S.nbt.values()) == {2 if S.cfg == "S" else 1}, S.nbt          # the dead projects included
    assert not bad, "\n".join(bad)


def test_pool_nodes(step):
    S = step
    bad = S.bad_pools + _report(S, "lazy pools")
    assert not bad, "\n".join(bad)


def test_deconv_nodes(step):
    bad = _report_conv(step, ["deconv"])
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ coverage
def test_the_matrix_covers_every_producer_path_and_node(golden_sd):
    """coverage shown, not assumed, across the whole matrix (a case that has not run yet in this session runs here): every
    statistics producer the plans name has a chain length (one without raises KeyError when its case is evaluated) and a
    figure per BatchNorm it feeds in every statistics class -- the row family, the tilings, the fp16-pipe stem and chan_reduce
    among them (wres has a chain length but no plan of the matrix chooses it for a forward layer: see MEASURED); both bn_finalize paths ran, the double one exactly for the BatchNorms with 2048 partial rows or
    more, which the shapes put at the layers with one partial per output row of 8x256x96; conv, pool and deconv each read a
    lazy and a stored input; every node of the graph was compared in every case"""
    for case in CASES:
        if case not in _DONE:
            with pytest.MonkeyPatch.context() as mp:
                _DONE[case] = _run_step(case[0], case[1], golden_sd, mp)
    G = plan_graph()
    named, finalize, consumers = set(), set(), set()
    for case, S in _DONE.items():
        named |= {p[1] for p in S.producer.values()}
        for p in {q[1] for q in S.producer.values()}:          # each BatchNorm a producer feeds has a figure in all four classes
            fed = sum(q[1] == p for q in S.producer.values())
            for cls in ("batch mean", "batch var", "running_mean", "running_var"):
                assert sum("(%s, " % p in r[0] for r in S.ratio[cls]) == fed, (case, p, cls)
        finalize |= S.checked["finalize"]
        consumers |= S.checked["consumers"]
        assert S.checked["nodes"] == set(range(G.n_nodes)), (case, set(range(G.n_nodes)) - S.checked["nodes"])
        doubles = {bn for bn, p in S.producer.items() if p[3] == "double"}
        B, H, W = S.dims_in
        by_shape = {bn for bn, p in S.producer.items() if p[2] >= FOLD_MIN_NB}
        assert doubles == by_shape
        rows = {bn: B * H for bn, p in S.producer.items() if p[1] in ROW_PRODUCERS and p[0] in (0, 1)}      # stem, level0
        assert all(S.producer[bn][2] == r for bn, r in rows.items()), (case, rows)
        if B * H >= FOLD_MIN_NB:          # (elsewhere only a tiling the autotuner may prefer at full resolution could reach 2048 rows)
            assert doubles and set(rows) <= doubles, (case, doubles)
        if S.cfg in ("D", "E", "S"):
            assert len(S.lazy) >= 30, (case, len(S.lazy))
        if S.cfg in ("A", "B", "C", "Z32"):
            assert not S.lazy, (case, S.lazy)
        if S.cfg == "E":
            assert G.feat in S.lazy
    _say("producers %s; finalize %s; consumers %s" % (sorted(named), sorted(finalize), sorted(consumers)))
    assert named <= set(PATCH_PRODUCERS + ROW_PRODUCERS) | {"chan_reduce"}, named      # (a new one raises in _chain_length first)
    assert {"chan_reduce", "stem_f16"} <= named and named & set(PATCH_PRODUCERS) and named & {"row", "row_lazy", "thin16"}, named
    assert finalize == {"float", "double"}
    assert consumers == {(k, s) for k in ("conv", "pool", "deconv") for s in ("lazy", "stored")}, consumers
