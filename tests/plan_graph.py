"""The network graph as the tests see it, the stressed state, and the layer-local backward, forward and eval references.

A plain module (no fixtures): `test_hip_operand_scale.py` (forward, layer by layer), `test_hip_backward_layers.py` (backward,
layer by layer), `test_backward_reference_cpu.py` (the checker checked against autograd), `test_hip_forward_layers.py` (the
train forward with its statistics, layer by layer), `test_forward_reference_cpu.py` (that checker checked against the oracle),
`test_hip_eval_layers.py` (the eval plan, layer by layer) and `test_eval_reference_cpu.py` (that checker checked against the
oracle) share it.

The graph mirrors mc_api.hip `build_net` / mc_train_plan.hip: node 0 is the stem's output, every live conv + BatchNorm, every
2x2 max-pool and every depthwise deconv makes one node, in forward order.

The backward reference (`backward_reference`) is pure torch on the CPU in float64.  It never differentiates through more than
ONE layer: every quantity of a layer is formed from the plan's own buffers around it, so no ReLU or max-pool decision can flip
and nothing is amplified.  The buffers, as `mc_train_debug_node` hands them out after a backward with MONOCON_HIP_GRAD_POOL=0:

    act[n]   the activation of node n (which = 0)
    g[n]     conv + BatchNorm node: dY, the gradient wrt the RAW conv output (the affine pass writes it in place over dZ)
             pool / deconv output node: dZ, the plain sum of its consumers' data gradients
             the stem (node 0): dY like every conv node -- except where the stem weight gradient forms dY on the fly
             (f16x2, MONOCON_HIP_STEM_FUSE=1, statistics left by level0's data-gradient epilogue): then the affine pass is
             skipped and the buffer keeps d = dZ * [z > 0], the masked gradient.  With STEM_FUSE=0, in fp32 / bf16x3, or with
             MONOCON_HIP_BM_EPILOGUE=0 it holds dY.
"""
import contextlib
import math
import os
import sys
import tempfile

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "monocon-pytorch_amd")
for _p in (PKG, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STRESS_SEED = 1234
STEM = "backbone.base_layer.0"
EPS = 1e-5


# ------------------------------------------------------------------------------------------------ the stressed state
def _bn_of(conv):
    """BatchNorm behind a train-plan conv (mc_api.hip build_net)"""
    if conv.endswith(".project.0") or conv.endswith("level0.0") or conv.endswith("level1.0") or conv.endswith("base_layer.0"):
        return conv[:-1] + "1"
    if conv.endswith(".root.conv"):
        return conv[:-len("conv")] + "bn"
    if conv.endswith(".conv1") or conv.endswith(".conv2"):
        return conv[:-len("convN")] + "bn" + conv[-1]
    assert conv.endswith(".conv") and ".ida_" in conv, conv
    return conv[:-len("conv")] + "bn1"


def stressed_state_dict(sd, seed=STRESS_SEED):
    """The golden state with (a) every conv in front of a train-mode BatchNorm rescaled per output channel, log-uniformly
    over [1, 10^3] (running statistics rescaled with it: the network's function does not change), and (b) every such
    BatchNorm's gamma log-uniform over [1e-2, 10] and beta uniform over [-3, 10] -- off-centre channels of both signs."""
    g = torch.Generator().manual_seed(seed)
    out = {k: v.clone() for k, v in sd.items()}
    for conv, _ in _plan_convs():
        w = out[conv + ".weight"]
        bn = _bn_of(conv)
        C = w.shape[0]
        s = 10.0 ** (3.0 * torch.rand(C, generator=g, dtype=torch.float64))
        out[conv + ".weight"] = (w.double() * s[:, None, None, None]).float()
        out[bn + ".running_mean"] = (out[bn + ".running_mean"].double() * s).float()
        out[bn + ".running_var"] = (out[bn + ".running_var"].double() * s * s).float()
        out[bn + ".weight"] = (10.0 ** (-2.0 + 3.0 * torch.rand(C, generator=g, dtype=torch.float64))).float()
        out[bn + ".bias"] = (-3.0 + 13.0 * torch.rand(C, generator=g, dtype=torch.float64)).float()
    return out


def stressed_batch(seed, B, H, W):
    """(c) frames with a strong DC offset after Normalize: alternately a bright and a dark frame with faint texture"""
    from hipmonocon import synth
    batch = synth.make_batch(seed, B, H, W)
    img = batch["img"]
    for b in range(B):
        img[b] = (2.1 if b % 2 == 0 else -1.9) + 0.05 * img[b]
    return batch


# ------------------------------------------------------------------------------------------------ the train plan's graph
class PlanGraph:
    """recs: per live conv layer (conv name, source nodes, residual node or -1, relu, output node, kernel size, stride);
    pools: (input node, output node); deconvs: (parameter name `neck.ida_i.up_t`, input node, output node);
    steps: all of them in forward order, ("conv", rec) / ("pool", in, out) / ("deconv", name, in, out);
    node_c / node_down: channels and down-scale of every node (node 0: 16 channels at full resolution);
    dead: (conv name, source node) of the outer `project` convs of the two-level trees: no node, their statistics still tick;
    consumers[n]: who reads node n, in the order the BACKWARD writes their shares into n's gradient (records in reverse
    forward order; within a conv record the residual's share -- written by the BatchNorm backward -- before the data gradients
    of its sources in source order): ("conv", rec, source index, channel offset) / ("res", rec) / ("pool", out) /
    ("deconv", name, out)."""

    def __init__(self):
        self.recs, self.pools, self.deconvs, self.steps = [], [], [], []
        self.node_c, self.node_down = [16], [1]
        self.feat = -1
        self.levels = []          # the nodes of the backbone's level outputs l0 .. l5
        self.dead = []            # (conv name, source node) of the outer `project` convs: never consumed, statistics still tick

    @property
    def n_nodes(self):
        return len(self.node_c)

    def dims(self, B, H, W):
        return [(B, c, H // d, W // d) for c, d in zip(self.node_c, self.node_down)]

    @property
    def consumers(self):
        cons = [[] for _ in range(self.n_nodes)]
        for st in reversed(self.steps):
            if st[0] == "conv":
                rec = st[1]
                if rec[2] >= 0:
                    cons[rec[2]].append(("res", rec))
                off = 0
                for i, s in enumerate(rec[1]):
                    cons[s].append(("conv", rec, i, off))
                    off += self.node_c[s]
            elif st[0] == "pool":
                cons[st[1]].append(("pool", st[2]))
            else:
                cons[st[2]].append(("deconv", st[1], st[3]))
        return cons


def plan_graph():
    """The node order of the train plan (mc_train_plan.hip: stem, conv_bn, pool, deconv, tree and the neck loop)"""
    from hipmonocon import netspec
    shapes = netspec.state_shapes()
    G = PlanGraph()
    pooled = {}

    def node(c, down):
        G.node_c.append(c)
        G.node_down.append(down)
        return G.n_nodes - 1

    def conv_bn(name, ks, stride, srcs, res, relu, dead=False):
        if dead:
            G.dead.append((name, srcs[0]))
            return -1
        cout = shapes[name + ".weight"][0][0]
        assert shapes[name + ".weight"][0][1] == sum(G.node_c[s] for s in srcs), name
        o = node(cout, G.node_down[srcs[0]] * stride)
        rec = (name, list(srcs), res, relu, o, ks, stride)
        G.recs.append(rec)
        G.steps.append(("conv", rec))
        return o

    def pool(x):
        if x not in pooled:
            pooled[x] = node(G.node_c[x], G.node_down[x] * 2)
            G.pools.append((x, pooled[x]))
            G.steps.append(("pool", x, pooled[x]))
        return pooled[x]

    def block(n, x, residual, stride):
        y = conv_bn(n + ".conv1", 3, stride, [x], -1, True)
        return conv_bn(n + ".conv2", 3, 1, [y], residual if residual >= 0 else x, True)

    def tree(n, levels, cin, cout, stride, level_root, x, children):
        bottom = pool(x) if stride > 1 else x
        if level_root:
            children = children + [bottom]
        if levels == 1:
            residual = bottom
            if cin != cout:
                residual = conv_bn(n + ".project.0", 1, 1, [bottom], -1, False)
            x1 = block(n + ".tree1", x, residual, stride)
            x2 = block(n + ".tree2", x1, -1, 1)
            return conv_bn(n + ".root.conv", 1, 1, [x2, x1] + children, -1, True)
        if cin != cout:
            conv_bn(n + ".project.0", 1, 1, [bottom], -1, False, dead=True)
        x1 = tree(n + ".tree1", levels - 1, cin, cout, stride, False, x, [])
        return tree(n + ".tree2", levels - 1, cout, cout, 1, False, x1, children + [x1])

    l0 = conv_bn("backbone.level0.0", 3, 1, [0], -1, True)
    l1 = conv_bn("backbone.level1.0", 3, 2, [l0], -1, True)
    l2 = tree("backbone.level2", 1, 32, 64, 2, False, l1, [])
    l3 = tree("backbone.level3", 2, 64, 128, 2, True, l2, [])
    l4 = tree("backbone.level4", 2, 128, 256, 2, True, l3, [])
    l5 = tree("backbone.level5", 1, 256, 512, 2, True, l4, [])
    G.levels = [l0, l1, l2, l3, l4, l5]
    layers = [l2, l3, l4, l5]
    for i in range(3):
        j = 4 - i - 2
        for t in range(1, 4 - j):
            pre = "neck.ida_%d." % i
            p = conv_bn(pre + "proj_%d.conv" % t, 3, 1, [layers[j + t]], -1, True)
            u = node(G.node_c[p], G.node_down[p] // 2)           # the depthwise deconv of p
            G.deconvs.append((pre + "up_%d" % t, p, u))
            G.steps.append(("deconv", pre + "up_%d" % t, p, u))
            layers[j + t] = conv_bn(pre + "node_%d.conv" % t, 3, 1, [layers[j + t - 1], u], -1, True)
    G.feat = layers[3]
    return G


def _plan_graph():
    """(conv records, number of nodes): see PlanGraph"""
    G = plan_graph()
    return G.recs, G.n_nodes


def _plan_convs():
    """(conv, bn) of every conv in front of a train-mode BatchNorm, the stem included (dead `project` convs too: they
    still tick their statistics)"""
    names = [STEM] + [r[0] for r in _plan_graph()[0]]
    from hipmonocon import netspec
    shapes = netspec.state_shapes()
    for k in shapes:                                     # the outer `project` of the two-level trees (never consumed)
        if k.endswith(".project.0.weight") and k[:-len(".weight")] not in names:
            names.append(k[:-len(".weight")])
    return [(n, _bn_of(n)) for n in names]


def layer_kind(ks, stride):
    return "stem" if ks == 7 else ("1x1" if ks == 1 else "3x3s%d" % stride)


# ------------------------------------------------------------------------------------------------ running a plan
def _model(sd, precision):
    from model import MonoConDetector
    m = MonoConDetector(34, pretrained_backbone=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().train().set_precision(precision)


@contextlib.contextmanager
def stderr_lines():
    """what the library writes to file descriptor 2 inside the block (the plan's `[plan]` debug lines), as a list of lines
    filled on exit (capfd is function-scoped; the step fixtures are module-scoped)"""
    lines = []
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            yield lines
        finally:
            sys.stderr.flush()
            os.dup2(keep, 2)
            os.close(keep)
            f.seek(0)
            lines += f.read().decode(errors="replace").splitlines()


def _node_dims(m, i):
    import ctypes as C
    eng = m._engine()
    dims = (C.c_int * 4)()
    assert eng.lib.mc_train_debug_node(eng.h, int(i), 0, None, dims, None) == 0
    return tuple(dims)


def _read_node(m, i, which=0):
    """node i of the model's train plan (NCHW float32); a lazy node is formed without changing the plan"""
    import ctypes as C
    eng = m._engine()
    dims = (C.c_int * 4)()
    assert eng.lib.mc_train_debug_node(eng.h, int(i), int(which), None, dims, None) == 0
    out = torch.empty(tuple(dims), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = eng.lib.mc_train_debug_node(eng.h, int(i), int(which), C.c_void_p(out.data_ptr()), dims, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu()


# ------------------------------------------------------------------------------------------------ the backward reference
def _floored(M):
    """the magnitude sum of a tensor, floored at 2^-10 of its maximum (dead channels do not divide by zero)"""
    return M.clamp_min(max(float(M.max()), 1e-300) * 2.0 ** -10)


def _conv_step(xs, w, gout, ks, stride, dtype, absolute=False):
    """ONE conv layer differentiated on its own: (y, dW, [data gradient of every source]) for the upstream gradient `gout`;
    absolute: the same sums over absolute values (the magnitude every rounding error is relative to)"""
    def cv(t):
        t = t.detach().to(dtype)          # (detach: a fresh tensor object, the caller's never turns into a leaf)
        return t.abs() if absolute else t
    xs = [cv(x).requires_grad_(True) for x in xs]
    w = cv(w).requires_grad_(True)
    y = F.conv2d(torch.cat(xs, 1) if len(xs) > 1 else xs[0], w, stride=stride, padding=ks // 2)
    grads = torch.autograd.grad(y, [w] + xs, cv(gout))
    return y.detach(), grads[0], list(grads[1:])


def _pool_bwd(x, gout, dtype, absolute=False):
    """max_pool2d(2) backward: a cast keeps ties, and torch routes to the first maximum in scan order, as the kernel does"""
    x = x.detach().to(dtype).requires_grad_(True)
    gout = gout.detach().to(dtype)
    return torch.autograd.grad(F.max_pool2d(x, 2), x, gout.abs() if absolute else gout)[0]


def _deconv_step(x, w, gout, dtype, absolute=False):
    """depthwise ConvTranspose2d(k 4, s 2, p 1, groups C) differentiated on its own: (weight gradient, input gradient)"""
    def cv(t):
        t = t.detach().to(dtype)          # (detach: a fresh tensor object, the caller's never turns into a leaf)
        return t.abs() if absolute else t
    x, w = cv(x).requires_grad_(True), cv(w).requires_grad_(True)
    u = F.conv_transpose2d(x, w, stride=2, padding=1, groups=x.shape[1])
    gw, gx = torch.autograd.grad(u, [w, x], cv(gout))
    return gw, gx


class Triple:
    """a reference quantity: fp64 value, fp64 magnitude sum, and (yard-stick) the same quantity carried out in float32"""
    __slots__ = ("ref", "mag", "f32")

    def __init__(self, ref=None, mag=None, f32=None):
        self.ref, self.mag, self.f32 = ref, mag, f32

    def add(self, ref, mag, f32=None):
        self.ref = ref if self.ref is None else self.ref + ref
        self.mag = mag if self.mag is None else self.mag + mag
        if f32 is not None:
            self.f32 = f32 if self.f32 is None else self.f32 + f32          # float32, in the order the plan adds its shares

    def floored(self):
        return _floored(self.mag)

    def err(self, got):
        """elementwise |got - ref| / M"""
        return (got.double() - self.ref).abs() / _floored(self.mag)

    def f32_err(self):
        return float(((self.f32.double() - self.ref).abs() / _floored(self.mag)).max())


class BackwardReference:
    """what `backward_reference` found: per conv name `dW` (Triple) and `bn` (dict: dbeta, dgamma, their |term| sums, n,
    mean, rstd, a = gamma * rstd); per node `dZ` (Triple: the sum of its consumers' shares), `d` (the masked dZ, conv nodes),
    `dY` (conv nodes), `y` (the fp64 raw conv output) and `ymag` (sum |x| |w|); per deconv name `dWup` (Triple)."""

    def __init__(self, graph):
        self.graph = graph
        self.dW, self.dWup, self.bn = {}, {}, {}
        self.dZ, self.d, self.dY, self.y, self.ymag, self.tmax = {}, {}, {}, {}, {}, {}


def backward_reference(graph, act, g, img, sd, yardstick=True):
    """The layer-local backward of backbone + neck in float64 from the plan's own buffers (see the module docstring for what
    `act` and `g` hold).  Covered: every live conv layer (the dead `project` convs are not in the graph); for `feat`, whose
    dZ comes from the head backward, only the weight-gradient identity.

        dW_L  = conv2d_weight(cat(act[srcs]), g[o])                  (the plan's weight gradient reads this same dY)
        dZ_o  = sum over o's consumers, in plan order, of
                  conv consumer C, source slice s:  conv2d_input(g[out(C)], W_C) restricted to the slice
                  residual consumer R:              d_R (below, recursively)
                  pool consumer:                    max_pool2d backward of g[pool node] on act[o]
                  deconv consumer:                  input gradient of the depthwise conv_transpose2d against g[u]
        d_o   = dZ_o * (act[o] > 0) where the layer has a ReLU: the GPU's own mask
        y     = conv2d(cat(act[srcs]), W) with its batch statistics;  dbeta = sum d, dgamma = sum d * yhat,
        dY_o  = gamma * rstd * (d - mean d - yhat * mean(d * yhat))
        dWup  = depthwise conv_transpose2d weight gradient from act[in] and g[u]
        stem:   d_0 from level0's share; dW from the image and the fp64 dY_0 (NOT from g[0], whose content depends on the path)

    yardstick: also every conv quantity in float32 from the same float32 buffers, shares added in the plan's order."""
    R = BackwardReference(graph)
    D = torch.float64
    dZ = {n: Triple() for n in range(graph.n_nodes)}
    R.dZ = dZ

    def bn_backward(name, o, xs, relu, ks, stride):
        """d, statistics and dY of the conv layer `name` with output node o, from its complete dZ"""
        w = sd[name + ".weight"].double()
        bn = _bn_of(name)
        gamma = sd[bn + ".weight"].double()
        x = torch.cat([t.double() for t in xs], 1)
        y = F.conv2d(x, w, stride=stride, padding=ks // 2)
        R.ymag[o] = F.conv2d(x.abs(), w.abs(), stride=stride, padding=ks // 2)
        # the f16x2 operand-split scale of the layer: sum over sources of max |x_s| * sum |w_c,s| (test_hip_operand_scale)
        tm, c0 = torch.zeros_like(gamma), 0
        for t in xs:
            tm += float(t.abs().max()) * w[:, c0:c0 + t.shape[1]].abs().sum((1, 2, 3))
            c0 += t.shape[1]
        R.tmax[o] = tm
        mask = (act[o] > 0).double() if relu else torch.ones_like(y)
        d = dZ[o].ref * mask
        n = y.numel() // y.shape[1]
        mean = y.mean((0, 2, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(y.var((0, 2, 3), unbiased=False, keepdim=True) + EPS)
        yhat = (y - mean) * rstd
        dbeta, dgamma = d.sum((0, 2, 3)), (d * yhat).sum((0, 2, 3))
        a = gamma[None, :, None, None] * rstd
        R.d[o], R.y[o] = d, y
        R.dY[o] = a * (d - dbeta[None, :, None, None] / n - yhat * dgamma[None, :, None, None] / n)
        R.bn[name] = dict(dbeta=dbeta, dgamma=dgamma, n=n, mean=mean.flatten(), rstd=rstd.flatten(), a=a.flatten(), mask=mask,
                          abs_d=d.abs().sum((0, 2, 3)), abs_dy=(d * y).abs().sum((0, 2, 3)), yhat=yhat)
        return d, mask

    for st in reversed(graph.steps):
        if st[0] == "pool":
            _, i, o = st
            dZ[i].add(_pool_bwd(act[i], g[o], D), _pool_bwd(act[i], g[o], D, True),
                      _pool_bwd(act[i], g[o], torch.float32) if yardstick else None)
        elif st[0] == "deconv":
            _, name, i, o = st
            w = sd[name + ".weight"]
            gw, gx = _deconv_step(act[i], w, g[o], D)
            mw, mx = _deconv_step(act[i], w, g[o], D, True)
            fw, fx = _deconv_step(act[i], w, g[o], torch.float32) if yardstick else (None, None)
            R.dWup[name] = Triple(gw, mw, fw)
            dZ[i].add(gx, mx, fx)
        else:
            name, srcs, res, relu, o, ks, stride = st[1]
            xs = [act[s] for s in srcs]
            if o != graph.feat:
                d, mask = bn_backward(name, o, xs, relu, ks, stride)
                if res >= 0:
                    dZ[res].add(d, dZ[o].mag * mask, (dZ[o].f32 * mask.float()) if yardstick else None)
            w = sd[name + ".weight"]
            _, gw, gxs = _conv_step(xs, w, g[o], ks, stride, D)
            _, mw, mxs = _conv_step(xs, w, g[o], ks, stride, D, True)
            fw, fxs = None, [None] * len(srcs)
            if yardstick:
                _, fw, fxs = _conv_step(xs, w, g[o], ks, stride, torch.float32)
            R.dW[name] = Triple(gw, mw, fw)
            for s, gx, mx, fx in zip(srcs, gxs, mxs, fxs):
                dZ[s].add(gx, mx, fx)
    # the stem: node 0's dZ is level0's share; its weight gradient from the image and the fp64 dY
    act_img = {-1: img}
    bn_backward(STEM, 0, [act_img[-1]], True, 7, 1)
    wshape = sd[STEM + ".weight"].shape
    gw = torch.nn.grad.conv2d_weight(img.double(), wshape, R.dY[0], padding=3)
    mw = torch.nn.grad.conv2d_weight(img.double().abs(), wshape, R.dY[0].abs(), padding=3)
    fw = torch.nn.grad.conv2d_weight(img.float(), wshape, R.dY[0].float(), padding=3) if yardstick else None
    R.dW[STEM] = Triple(gw, mw, fw)
    return R


def norm_err(got, ref):
    """norm-wise error: max |got - ref| / max |ref|"""
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def compare_normwise(R, g, grads, stem_holds="dY"):
    """every compared quantity, norm-wise: {(class, layer or node): error}.  grads: parameter name -> gradient."""
    G = R.graph
    out = {}
    for name, t in R.dW.items():
        out[("dW", name)] = norm_err(grads[name + ".weight"], t.ref)
    for name, t in R.dWup.items():
        out[("dWup", name)] = norm_err(grads[name + ".weight"], t.ref)
    for name, b in R.bn.items():
        bn = _bn_of(name)
        out[("dgamma", name)] = norm_err(grads[bn + ".weight"], b["dgamma"])
        out[("dbeta", name)] = norm_err(grads[bn + ".bias"], b["dbeta"])
    for name, srcs, res, relu, o, ks, stride in G.recs:
        if o != G.feat:
            out[("dY", name)] = norm_err(g[o], R.dY[o])
    for _, o in G.pools:
        out[("dZ", "pool node %d" % o)] = norm_err(g[o], R.dZ[o].ref)
    for name, _, o in G.deconvs:
        out[("dZ", name)] = norm_err(g[o], R.dZ[o].ref)
    out[("stem g", STEM)] = norm_err(g[0], R.dY[0] if stem_holds == "dY" else R.d[0])
    return out


# ------------------------------------------------------------------------------------------------ the forward reference
BN_MOMENTUM = 0.1


class ForwardReference:
    """what `forward_reference` found.
    layers: [(kind, conv name, node, Triple)] for the stem and every live conv (`feat` included): z in fp64, its magnitude
      M = |a| conv2d(|x|, |w|) + |b| + |res| (unfloored; Triple.floored() floors it), the float32 yard-stick;
    pools: [(in, out, max_pool2d(act[in], 2, 2))]; deconvs: [(name, in, out, Triple)];
    stats[conv name] (dead `project` convs too), per channel unless said: n (a number), K (terms per output), mean, var (biased),
      shift (the running mean before the step), m0 = mean - shift, e1 = E|y - shift|, e2 = E[(y - shift)^2], a, b, tmax (the
      operand-split scale T_c), ymag = conv2d(|x|, |w|) (the whole map) and ymag_max, its maximum over the map, node; live
      layers also dev = |y - mean| and zmag = |a| |y| + |b| (whole maps: the size of a y + b before residual and ReLU);
    running[bn name]: rm, rv (Triple: the fp64 update, its magnitude sum (1 - m) |old| + m |statistic|, the float32
      yard-stick's buffer), nbt (num_batches_tracked after the step)"""

    def __init__(self, graph):
        self.graph = graph
        self.layers, self.pools, self.deconvs, self.stats, self.running = [], [], [], {}, {}


def forward_reference(graph, act, img, sd_before, yardstick=True):
    """The layer-local train-mode forward of backbone + neck in float64 from the plan's own buffers: `act[n]` is node n as
    `mc_train_debug_node(which = 0)` hands it out AFTER the forward, `sd_before` the state the forward started from (its
    running means are also the shift of the kernels' variance sums).  No quantity goes through more than ONE layer:

        conv node    y = conv2d(cat(act[srcs]), W) (the stem: of img), biased batch mean / var over (B, H, W),
                     a = gamma / sqrt(var + eps), b = beta - mean a, z = a y + b (+ act[res]), clamped at 0 under a ReLU
        pool node    max_pool2d(act[in], 2, 2), in the precision of act[in]: a maximum rounds nothing
        deconv node  the depthwise conv_transpose2d of act[in], magnitude from |x|, |w|
        running      rm' = (1 - m) rm + m mean, rv' = (1 - m) rv + m var n / (n - 1), m = 0.1, for every BatchNorm of
                     `_plan_convs()`: the dead outer `project` convs read their `bottom` pool node (graph.dead)

    yardstick: the same conv node by torch in float32 from the same float32 buffers -- F.conv2d, then
    F.batch_norm(training=True) on copies of the running buffers, which are the yard-stick's running buffers."""
    R = ForwardReference(graph)
    D, S = torch.float64, torch.float32
    m = BN_MOMENTUM
    v = lambda t: t[None, :, None, None]          # noqa: E731

    def conv_bn(rec, xs, live=True):
        name, srcs, res, relu, o, ks, stride = rec
        bn = _bn_of(name)
        w = sd_before[name + ".weight"].to(D)
        gamma, beta = sd_before[bn + ".weight"].to(D), sd_before[bn + ".bias"].to(D)
        rm, rv = sd_before[bn + ".running_mean"].to(D), sd_before[bn + ".running_var"].to(D)
        x = torch.cat([t.to(D) for t in xs], 1)
        y = F.conv2d(x, w, stride=stride, padding=ks // 2)
        ymag = F.conv2d(x.abs(), w.abs(), stride=stride, padding=ks // 2)
        tm, c0 = torch.zeros_like(gamma), 0
        for t in xs:          # the f16x2 operand-split scale, as bn_backward's tmax
            tm += float(t.abs().max()) * w[:, c0:c0 + t.shape[1]].abs().sum((1, 2, 3))
            c0 += t.shape[1]
        n = y.numel() // y.shape[1]
        mean = y.mean((0, 2, 3))
        var = y.var((0, 2, 3), unbiased=False)
        a = gamma / torch.sqrt(var + EPS)
        b = beta - mean * a
        ys = y - v(rm)
        R.stats[name] = dict(n=n, K=w[0].numel(), mean=mean, var=var, shift=rm, m0=mean - rm, e1=ys.abs().mean((0, 2, 3)),
                             e2=(ys * ys).mean((0, 2, 3)), a=a, b=b, tmax=tm, ymag=ymag, ymag_max=ymag.amax((0, 2, 3)),
                             dev=(y - v(mean)).abs() if live else None, zmag=v(a.abs()) * y.abs() + v(b.abs()) if live else None,
                             node=o if live else None)
        unb = var * n / (n - 1)
        run = dict(rm=Triple((1 - m) * rm + m * mean, (1 - m) * rm.abs() + m * mean.abs()),
                   rv=Triple((1 - m) * rv + m * unb, (1 - m) * rv.abs() + m * unb),
                   nbt=int(sd_before[bn + ".num_batches_tracked"]) + 1)
        R.running[bn] = run
        z32 = None
        if yardstick:
            rm32, rv32 = sd_before[bn + ".running_mean"].to(S).clone(), sd_before[bn + ".running_var"].to(S).clone()
            y32 = F.conv2d(torch.cat([t.to(S) for t in xs], 1), sd_before[name + ".weight"].to(S), stride=stride, padding=ks // 2)
            z32 = F.batch_norm(y32, rm32, rv32, sd_before[bn + ".weight"].to(S), sd_before[bn + ".bias"].to(S), True, m, EPS)
            run["rm"].f32, run["rv"].f32 = rm32, rv32
        if not live:
            return
        z = v(a) * y + v(b)
        M = v(a.abs()) * ymag + v(b.abs())
        if res >= 0:
            z, M = z + act[res].to(D), M + act[res].to(D).abs()
            if yardstick:
                z32 = z32 + act[res].to(S)
        if relu:
            z = z.clamp_min(0)
            z32 = z32.clamp_min(0) if yardstick else None
        R.layers.append((layer_kind(ks, stride), name, o, Triple(z, M, z32)))

    conv_bn(STEM_REC, [img])
    for st in graph.steps:
        if st[0] == "conv":
            conv_bn(st[1], [act[s] for s in st[1][1]])
        elif st[0] == "pool":
            R.pools.append((st[1], st[2], F.max_pool2d(act[st[1]], 2, 2)))
        else:
            _, name, i, o = st
            R.deconvs.append((name, i, o, Triple(eval_deconv(sd_before, name, act[i], D), eval_deconv(sd_before, name, act[i], D, True),
                                                 eval_deconv(sd_before, name, act[i], S) if yardstick else None)))
    for name, src in graph.dead:
        conv_bn((name, [src], -1, False, -1, 1, 1), [act[src]], live=False)
    return R


# ------------------------------------------------------------------------------------------------ the eval plan
# The eval plan (mc_api.hip get_plan) runs the same graph with the same node ids; `mc_infer_debug_node` reads it after a
# forward: every node, the raw hidden map of the fused head conv, head_attn_kernel's AttnBN affine and its statistic s.
# `eval_reference` is the layer-local fp64 reference of that forward: like the backward reference it never computes more than
# ONE layer from the plan's own buffers, so no ReLU, max-pool or clamp decision of an earlier layer can flip.
U24 = 2.0 ** -24
ABN_EPS = 1e-3
LOGIT_CLAMP = math.log(9999.0)          # sigmoid(x) = 1e-4 at -ln 9999, 1 - 1e-4 at +ln 9999
HEADS = ("heatmap_head", "wh_head", "offset_head", "center2kpt_offset_head", "kpt_heatmap_head", "kpt_heatmap_offset_head",
         "dim_head", "depth_head", "dir_feat")
HEAD_OUT = {"heatmap_head": [("center_heatmap_pred", "head.heatmap_head.3")], "wh_head": [("wh_pred", "head.wh_head.3")],
            "offset_head": [("offset_pred", "head.offset_head.3")],
            "center2kpt_offset_head": [("center2kpt_offset_pred", "head.center2kpt_offset_head.3")],
            "kpt_heatmap_head": [("kpt_heatmap_pred", "head.kpt_heatmap_head.3")],
            "kpt_heatmap_offset_head": [("kpt_heatmap_offset_pred", "head.kpt_heatmap_offset_head.3")],
            "dim_head": [("dim_pred", "head.dim_head.3")], "depth_head": [("depth_pred", "head.depth_head.3")],
            "dir_feat": [("alpha_cls_pred", "head.dir_cls.0"), ("alpha_offset_pred", "head.dir_reg.0")]}
HEAT_KEYS = ("center_heatmap_pred", "kpt_heatmap_pred")
STEM_REC = (STEM, [-1], -1, True, 0, 7, 1)            # the stem as a conv record: its source "node -1" is the image
EVAL_KINDS = ("stem", "3x3s1", "3x3s2", "1x1", "deconv", "head hidden")


def heat_clamps():
    """(floor, ceiling) of a float32 heat map: what the reference's clamp(sigmoid(x), 1e-4, 1 - 1e-4) saturates at"""
    lo, hi = torch.clamp(torch.tensor([-1.0, 2.0], dtype=torch.float32), 1e-4, 1.0 - 1e-4)
    return lo, hi


def _bn_params(sd, bn, dtype):
    return [sd[bn + k].to(dtype) for k in (".weight", ".bias", ".running_mean", ".running_var")]


def eval_conv(sd, rec, nodes, dtype, batch_norm=None):
    """one conv layer of the eval forward from `nodes`: conv of the source nodes, eval BatchNorm in the unfolded form
    gamma (x - rm) / sqrt(rv + eps) + beta (batch_norm: a callable (y, gamma, beta, rm, rv) in its place), residual, ReLU"""
    name, srcs, res, relu, o, ks, stride = rec
    x = torch.cat([nodes[s].to(dtype) for s in srcs], 1)
    y = F.conv2d(x, sd[name + ".weight"].to(dtype), stride=stride, padding=ks // 2)
    g, b, rm, rv = _bn_params(sd, _bn_of(name), dtype)
    v = lambda t: t[None, :, None, None]          # noqa: E731
    if batch_norm is not None:
        z = batch_norm(y, g, b, rm, rv)
    else:
        z = v(g) * (y - v(rm)) / torch.sqrt(v(rv) + EPS) + v(b)
    if res >= 0:
        z = z + nodes[res].to(dtype)
    return z.clamp_min(0) if relu else z


def eval_conv_mag(sd, rec, nodes):
    """(M, split): M = |scale_c| conv(|x|, |w|) + |shift_c| + |res| in fp64 with the folded scale = gamma / sqrt(rv + eps),
    shift = beta - rm scale; split = 2^-21 T_c |scale_c| per channel, the f16x2 operand-split term with T_c = sum over the
    sources of max |x_s| sum |w_c,s| (test_hip_operand_scale)"""
    name, srcs, res, relu, o, ks, stride = rec
    D = torch.float64
    w = sd[name + ".weight"].to(D).abs()
    x = torch.cat([nodes[s].to(D).abs() for s in srcs], 1)
    g, b, rm, rv = _bn_params(sd, _bn_of(name), D)
    scale = g / torch.sqrt(rv + EPS)
    shift = b - rm * scale
    M = scale.abs()[None, :, None, None] * F.conv2d(x, w, stride=stride, padding=ks // 2) + shift.abs()[None, :, None, None]
    if res >= 0:
        M = M + nodes[res].to(D).abs()
    tm, c0 = torch.zeros_like(g), 0
    for s in srcs:
        cs = nodes[s].shape[1]
        tm += float(nodes[s].abs().max()) * w[:, c0:c0 + cs].sum((1, 2, 3))
        c0 += cs
    return M, 2.0 ** -21 * tm * scale.abs()


def eval_deconv(sd, name, x, dtype, absolute=False):
    """the depthwise ConvTranspose2d(k 4, s 2, p 1, groups C) of the neck"""
    x, w = x.to(dtype), sd[name + ".weight"].to(dtype)
    if absolute:
        x, w = x.abs(), w.abs()
    return F.conv_transpose2d(x, w, stride=2, padding=1, groups=x.shape[1])


def head_hidden(sd, feat, dtype, absolute=False):
    """the fused head conv: the nine 3x3 64 -> 64 convs side by side, bias added (576 channels, head-major)"""
    w = torch.cat([sd["head.%s.0.weight" % h] for h in HEADS], 0).to(dtype)
    b = torch.cat([sd["head.%s.0.bias" % h] for h in HEADS], 0).to(dtype)
    x = feat.to(dtype)
    if absolute:
        x, w, b = x.abs(), w.abs(), b.abs()
    return F.conv2d(x, w, b, padding=1)


def attn_affine(sd, hidden, dtype, biased=False):
    """AttnBN in eval mode as one affine per (image, head, channel), following the oracle's `_attn_bn`
    (attentive_norm.py:79-91,154-164): y = g (x - rm) / sqrt(rv + 1e-3) + b = scale x + shift.
    -> dict: scale, shift (B, 9, 64); unit_scale = sum_k |y_k| |weight_k,c| / sqrt(rv + 1e-3) and
    unit_shift = sum_k |y_k| |bias_k,c| + |rm| unit_scale (what their rounding errors are relative to); s (B, 9, 64), the
    statistic mean / sqrt(var + 1e-3) with the UNBIASED variance (biased=True: the defect of the negative control); ratio:
    (mean - rm)^2 / (var + 1e-3), what the kernel's shifted one-pass sums cancel by"""
    out = {k: [] for k in ("scale", "shift", "unit_scale", "unit_shift", "s", "ratio")}
    B = hidden.shape[0]
    for hd, head in enumerate(HEADS):
        n = "head.%s.1" % head
        x = hidden[:, 64 * hd:64 * hd + 64].to(dtype)
        var, mean = torch.var_mean(x, dim=(2, 3), keepdim=True, unbiased=not biased)
        s = mean * (var + ABN_EPS).rsqrt()
        a = F.conv2d(s, sd[n + ".attn_weights.attention.0.weight"].to(dtype))
        g, b, rm, rv = _bn_params(sd, n + ".attn_weights.attention.1", dtype)
        a = F.batch_norm(a, rm, rv, g, b, False, 0.0, EPS)
        y = (F.relu6(a + 3.0) / 6.0).view(B, -1)
        wg, wb = sd[n + ".weight_"].to(dtype), sd[n + ".bias_"].to(dtype)
        rm, rv = sd[n + ".running_mean"].to(dtype), sd[n + ".running_var"].to(dtype)
        inv = (rv + ABN_EPS).rsqrt()
        scale = (y @ wg) * inv
        out["scale"].append(scale)
        out["shift"].append(y @ wb - rm * scale)
        us = (y.abs() @ wg.abs()) * inv
        out["unit_scale"].append(us)
        out["unit_shift"].append(y.abs() @ wb.abs() + rm.abs() * us)
        out["s"].append(s.view(B, 64))
        out["ratio"].append(((mean.view(B, 64) - rm) ** 2 / (var.view(B, 64) + ABN_EPS)))
    return {k: torch.stack(v, 1) for k, v in out.items()}


def head_outputs(sd, hidden, scale, shift, dtype):
    """the second head pass from (hidden, AttnBN scale, shift): h = relu(scale x + shift), the 65 rows of the 1x1 convs, the
    sigmoid-and-clamp epilogue of the two heat maps and the depth epilogue 1 / (sigmoid(v) + 1e-12) - 1 of depth row 0.
    -> (raw, out) per prediction key; dtype float64 also -> mag: M_row = sum_c |w_c| |h_c| + |b|"""
    raw, out, mag = {}, {}, {}
    for hd, head in enumerate(HEADS):
        x = hidden[:, 64 * hd:64 * hd + 64].to(dtype)
        h = (x * scale[:, hd, :, None, None].to(dtype) + shift[:, hd, :, None, None].to(dtype)).clamp_min(0)
        for key, conv in HEAD_OUT[head]:
            w, b = sd[conv + ".weight"].to(dtype), sd[conv + ".bias"].to(dtype)
            r = F.conv2d(h, w, b)
            raw[key] = r
            if dtype == torch.float64:
                mag[key] = F.conv2d(h.abs(), w.abs(), b.abs())
            if key in HEAT_KEYS:
                r = torch.clamp(torch.sigmoid(r), 1e-4, 1.0 - 1e-4)
            elif key == "depth_pred":
                r = torch.cat([1.0 / (torch.sigmoid(r[:, 0:1]) + 1e-12) - 1.0, r[:, 1:2]], 1)
            out[key] = r
    return (raw, out, mag) if dtype == torch.float64 else (raw, out)


class EvalReference:
    """what `eval_reference` found.  layers: [(kind, label, node or None, Triple, split)] for the stem, every live conv, every
    deconv and the head's hidden map (Triple: fp64 value, magnitude M, the float32 yard-stick; split: the per-channel f16x2
    operand-split term, None where there is none); pools: [(in, out)]; attn / attn32: `attn_affine` of HIP's hidden in fp64 /
    float32; raw, out, mag / raw32, out32: `head_outputs` of HIP's hidden and HIP's AttnBN affine in fp64 / float32"""

    def __init__(self, graph):
        self.graph, self.layers, self.pools = graph, [], []


def eval_reference(sd, G, nodes, hidden, attn, yardstick=True, stem=True):
    """The layer-local eval forward in float64 from the plan's own buffers.  nodes: {node id: float32 NCHW activation}, with
    the image as node -1; hidden: the fused head conv's raw output (B, 576, h, w); attn: (B, 2, 9, 64), HIP's AttnBN scale
    [:, 0] and shift [:, 1].

        stem, live convs   conv of the HIP source nodes, unfolded eval BatchNorm, residual, ReLU
        pools              listed only: the 2x2 max must be BIT-equal (`evaluate_eval`)
        deconvs            the depthwise 4x4 stride-2 transposed conv of the HIP input node
        head hidden        from node `feat`
        AttnBN             scale and shift from HIP's hidden, following the oracle's `_attn_bn`
        the ten maps       from HIP's hidden and HIP's scale and shift

    Every conv-like quantity comes with its magnitude M, the same operation on absolute values, floored at 2^-10 of the
    tensor maximum when it divides (Triple.floored).  yardstick: the same layer by torch in float32 from the same float32
    buffers (F.conv2d, unfolded F.batch_norm).  stem=False with a graph without steps: the head alone, from nodes[G.feat]."""
    R = EvalReference(G)
    D, S = torch.float64, torch.float32
    fbn = lambda y, g, b, rm, rv: F.batch_norm(y, rm, rv, g, b, False, 0.0, EPS)          # noqa: E731
    for st in ([("conv", STEM_REC)] if stem else []) + list(G.steps):
        if st[0] == "conv":
            rec = st[1]
            M, split = eval_conv_mag(sd, rec, nodes)
            t = Triple(eval_conv(sd, rec, nodes, D), M, eval_conv(sd, rec, nodes, S, fbn) if yardstick else None)
            R.layers.append((layer_kind(rec[5], rec[6]), rec[0], rec[4], t, split))
        elif st[0] == "pool":
            R.pools.append((st[1], st[2]))
        else:
            _, name, i, o = st
            t = Triple(eval_deconv(sd, name, nodes[i], D), eval_deconv(sd, name, nodes[i], D, True),
                       eval_deconv(sd, name, nodes[i], S) if yardstick else None)
            R.layers.append(("deconv", name, o, t, None))
    feat = nodes[G.feat]
    R.layers.append(("head hidden", "head.*.0", None, Triple(head_hidden(sd, feat, D), head_hidden(sd, feat, D, True),
                                                               head_hidden(sd, feat, S) if yardstick else None), None))
    R.attn = attn_affine(sd, hidden, D)
    R.attn32 = attn_affine(sd, hidden, S) if yardstick else None
    R.raw, R.out, R.mag = head_outputs(sd, hidden, attn[:, 0], attn[:, 1], D)
    if yardstick:
        R.raw32, R.out32 = head_outputs(sd, hidden, attn[:, 0], attn[:, 1], S)
    return R


class EvalFigures:
    """what `evaluate_eval` measured.  yard / gate / worst: per class; bad: per class, the lines of what missed its gate (empty:
    passed); rows: per class [(label, HIP error, float32 error, worst error / gate)]; excepted: per heat map, the share of
    positions within 8 U M_row of a clamp; split_needed: the conv layers that pass only with the operand-split term"""

    def __init__(self):
        self.yard, self.gate, self.worst, self.bad, self.rows, self.excepted = {}, {}, {}, {}, {}, {}
        self.split_needed = []

    def ratio(self, cls):
        """worst HIP error / float32 yard-stick of a class"""
        return self.worst[cls] / max(self.yard[cls], 1e-300)


def evaluate_eval(R, nodes, hidden, attn, maps, split_kinds=()):
    """The gates of test_hip_eval_layers.py (U = 2^-24), also run by the CPU test on float32 stand-ins for the kernels.

      conv kinds, deconv, head hidden: elementwise |got - ref| / M against 5 x (the float32 yard-stick's worst of the kind)
        + 4 U; for the kinds in `split_kinds` the f16x2 operand-split term 2^-21 T_c |scale_c| / M is added
      pools: bit-equal to max_pool2d of the input node
      AttnBN scale, shift: |got - ref| / unit against 5 x the float32 `attn_affine` + 4 U
      linear rows: |got - ref| / M_row against 5 x float32 + 4 U
      heat maps: the positions at the floor and at the ceiling are the reference's (its output rounded to float32 -- a float32
        map cannot show a value between the ceiling and its neighbour below), except where the fp64 raw logit lies within
        8 U M_row of +-ln 9999, at most 0.1 % of a map; every value: |got - ref| / (M_row / 4) against 5 x float32 + 4 U
      depth row 0: |got - ref| / ((1 + |d0|) (1 + M_row)) against 5 x float32 + 4 U"""
    Fg = EvalFigures()
    G = R.graph

    def gated(cls, items):
        """items: [(label, got, ref, float32, divisor, extra allowance in units of the divisor or None)]"""
        errs = [(label, (got.double() - ref).abs() / div, float(((f32.double() - ref).abs() / div).max()), extra)
                for label, got, ref, f32, div, extra in items]
        Fg.yard[cls] = max(e[2] for e in errs)
        Fg.gate[cls] = 5 * Fg.yard[cls] + 4 * U24
        Fg.worst[cls] = max(float(e[1].max()) for e in errs)
        Fg.rows[cls], Fg.bad[cls] = [], []
        for label, e, f, extra in errs:
            plain = float(e.max()) / Fg.gate[cls]
            r = plain if extra is None else float((e / (Fg.gate[cls] + extra)).max())
            if extra is not None and plain > 1.0 >= r:
                Fg.split_needed.append(label)
            Fg.rows[cls].append((label, float(e.max()), f, r))
            if not r <= 1.0:
                Fg.bad[cls].append("%s %s: %.3g of the gate (error %.3g, float32 %.3g)" % (cls, label, r, float(e.max()), f))

    for kind in EVAL_KINDS:
        items = []
        for k, label, o, t, split in R.layers:
            if k != kind:
                continue
            got = hidden if o is None else nodes[o]
            assert got.shape == t.ref.shape, (label, got.shape, t.ref.shape)
            extra = split[None, :, None, None] / t.floored() if (kind in split_kinds and split is not None) else None
            items.append((label, got, t.ref, t.f32, t.floored(), extra))
        if items:
            gated(kind, items)
    Fg.bad["pools"] = ["pool node %d of node %d is not bit-equal" % (o, i) for i, o in R.pools
                       if not torch.equal(F.max_pool2d(nodes[i], 2), nodes[o])]
    a, a32 = R.attn, R.attn32
    gated("AttnBN", [("scale", attn[:, 0], a["scale"], a32["scale"], a["unit_scale"].clamp_min(1e-300), None),
                     ("shift", attn[:, 1], a["shift"], a32["shift"], a["unit_shift"].clamp_min(1e-300), None)])
    lin = []
    for key in R.out:
        if key in HEAT_KEYS:
            continue
        sl = slice(1, 2) if key == "depth_pred" else slice(None)
        lin.append((key, maps[key][:, sl], R.out[key][:, sl], R.out32[key][:, sl], _floored(R.mag[key][:, sl]), None))
    gated("linear rows", lin)
    gated("heat maps", [(key, maps[key], R.out[key], R.out32[key], _floored(R.mag[key]) / 4, None) for key in HEAT_KEYS])
    lo, hi = heat_clamps()
    for key in HEAT_KEYS:
        got, ref32 = maps[key], R.out[key].float()
        near = ((R.raw[key].abs() - LOGIT_CLAMP).abs() <= 8 * U24 * R.mag[key])
        Fg.excepted[key] = float(near.double().mean())
        if Fg.excepted[key] > 1e-3:
            Fg.bad["heat maps"].append("%s: %.3g of the map within 8 U M_row of a clamp" % (key, Fg.excepted[key]))
        if float(got.min()) < float(lo) or float(got.max()) > float(hi):
            Fg.bad["heat maps"].append("%s: values outside [1e-4, 1 - 1e-4]" % key)
        for what, edge in (("floor", lo), ("ceiling", hi)):
            wrong = ((got == edge) != (ref32 == edge)) & ~near
            if bool(wrong.any()):
                Fg.bad["heat maps"].append("%s: %d positions differ from the reference's set at the %s" % (key, int(wrong.sum()), what))
    d0, m0 = R.out["depth_pred"][:, 0:1], R.mag["depth_pred"][:, 0:1]
    gated("depth row 0", [("depth_pred[0]", maps["depth_pred"][:, 0:1], d0, R.out32["depth_pred"][:, 0:1],
                           (1 + d0.abs()) * (1 + m0), None)])
    return Fg


def head_output_stress(sd, heat_gain=12.0, depth_gain=3.0):
    """the state with the 1x1 weights of the two heat-map heads scaled by `heat_gain` (the raw logits reach both clamps and the
    interior between them) and row 0 of depth_head.3, weight and bias, by `depth_gain` (the depth logit spans about +-15: d0
    from 1e-7 to 1e5)"""
    out = {k: v.clone() for k, v in sd.items()}
    for h in ("heatmap_head", "kpt_heatmap_head"):
        out["head.%s.3.weight" % h] = (sd["head.%s.3.weight" % h].double() * heat_gain).float()
    for k in ("weight", "bias"):
        t = out["head.depth_head.3." + k]
        t[0] = (t[0].double() * depth_gain).float()
    return out


def head_attention_stress(sd, gain=4.0):
    """the state with the gamma of every head's attention BatchNorm (head.*.1.attn_weights.attention.1.weight) scaled by `gain`:
    the hard sigmoid relu6(t + 3) / 6 of the AttnBN attention then sees inputs in all three of its regimes (t <= -3, the
    linear branch, t >= 3) instead of the linear one almost alone"""
    out = {k: v.clone() for k, v in sd.items()}
    n = 0
    for k in sd:
        if k.startswith("head.") and k.endswith(".1.attn_weights.attention.1.weight"):
            out[k] = (sd[k].double() * gain).float()
            n += 1
    assert n == len(HEADS), n
    return out


def head_decided_pixels(sd, hidden, tau=1e-4):
    """{head: (B, h, w) bool} from the heads' hidden maps (hidden[head]: the output of head.<head>.0, bias included): True
    where none of the head's 64 ReLU decisions after the train-mode AttnBN lies within tau of the channel's standard deviation
    of its threshold, by the oracle's own `_attn_bn` in the precision of `sd` and `hidden`"""
    from oracle import monocon_oracle as O
    out = {}
    with torch.no_grad():
        cx = O._Ctx(sd, True)
        for br, x in hidden.items():
            a = O._attn_bn(cx, x, "head.%s.1" % br)
            out[br] = (a.abs() / a.std(dim=(0, 2, 3), keepdim=True)).amin(dim=1) >= tau
    return out


# ---- reading the eval plan
def read_infer(eng, node, which=0):
    """mc_infer_debug_node on the engine's last eval plan: NCHW float32 on the host"""
    import ctypes as C
    dims = (C.c_int * 4)()
    rc = eng.lib.mc_infer_debug_node(eng.h, int(node), int(which), None, dims, None)
    assert rc == 0, eng.lib.mc_last_error(eng.h)
    out = torch.empty(tuple(dims), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = eng.lib.mc_infer_debug_node(eng.h, int(node), int(which), C.c_void_p(out.data_ptr()), dims, st)
    assert rc == 0, eng.lib.mc_last_error(eng.h)
    torch.cuda.synchronize()
    return out.cpu()
