"""The layer-local backward reference of `plan_graph.py` checked against torch autograd, without a GPU.

Backbone + neck are built from the graph records in float64 with autograd (train-mode BatchNorm, residuals, max_pool2d,
depthwise ConvTranspose2d) at 2x64x64 with random weights and a random upstream gradient at `feat`.  The autograd buffers are
handed to the reference in the GPU's layout (dY in conv nodes, dZ in pool and deconv nodes); every compared quantity must
come out within 1e-10 norm-wise -- that proves the consumer lists, the channel offsets and the formulas.  Three negative
controls prove the other direction: a wrong buffer or a wrong graph is flagged at the layer it touches.
"""
import pytest
import torch
import torch.nn.functional as F

from plan_graph import (EPS, STEM, PlanGraph, _bn_of, backward_reference, compare_normwise, plan_graph)

B, H, W = 2, 64, 64
TOL = 1e-10


def _random_state(graph, seed=11):
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, cout, cin, ks):
        sd[name + ".weight"] = torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) / (cin * ks * ks) ** 0.5
        bn = _bn_of(name)
        sd[bn + ".weight"] = 0.5 + torch.rand(cout, generator=g, dtype=torch.float64)
        sd[bn + ".bias"] = 0.3 * torch.randn(cout, generator=g, dtype=torch.float64)

    conv(STEM, 16, 3, 7)
    for name, srcs, res, relu, o, ks, stride in graph.recs:
        conv(name, graph.node_c[o], sum(graph.node_c[s] for s in srcs), ks)
    for name, i, o in graph.deconvs:
        sd[name + ".weight"] = 0.25 + 0.1 * torch.randn(graph.node_c[i], 1, 4, 4, generator=g, dtype=torch.float64)
    return sd


def _autograd_step(graph, sd, img, gfeat, drop_res=None):
    """forward + backward with autograd; drop_res: a conv name whose residual input is detached (its share never arrives).
    Returns act, g in the GPU's layout (dY in conv nodes, dZ in pool / deconv nodes) and the parameter gradients."""
    P = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    act, ys = {}, {}

    def conv_bn(name, x, ks, stride, res, relu):
        y = F.conv2d(x, P[name + ".weight"], stride=stride, padding=ks // 2)
        y.retain_grad()
        bn = _bn_of(name)
        mean = y.mean((0, 2, 3), keepdim=True)
        var = y.var((0, 2, 3), unbiased=False, keepdim=True)
        z = (y - mean) / torch.sqrt(var + EPS) * P[bn + ".weight"][None, :, None, None] + P[bn + ".bias"][None, :, None, None]
        if res is not None:
            z = z + res
        if relu:
            z = z.clamp_min(0)
        z.retain_grad()
        return y, z

    ys[0], act[0] = conv_bn(STEM, img, 7, 1, None, True)
    for st in graph.steps:
        if st[0] == "pool":
            act[st[2]] = F.max_pool2d(act[st[1]], 2)
            act[st[2]].retain_grad()
        elif st[0] == "deconv":
            x = act[st[2]]
            act[st[3]] = F.conv_transpose2d(x, P[st[1] + ".weight"], stride=2, padding=1, groups=x.shape[1])
            act[st[3]].retain_grad()
        else:
            name, srcs, res, relu, o, ks, stride = st[1]
            r = None
            if res >= 0:
                r = act[res].detach() if name == drop_res else act[res]
            ys[o], act[o] = conv_bn(name, torch.cat([act[s] for s in srcs], 1), ks, stride, r, relu)
    (act[graph.feat] * gfeat).sum().backward()
    conv_nodes = {0} | {r[4] for r in graph.recs}
    g = {n: (ys[n].grad if n in conv_nodes else act[n].grad).detach() for n in act}
    grads = {k: v.grad.detach() for k, v in P.items() if v.grad is not None}
    return {n: a.detach() for n, a in act.items()}, g, grads


@pytest.fixture(scope="module")
def setup():
    torch.manual_seed(5)
    graph = plan_graph()
    sd = _random_state(graph)
    img = torch.randn(B, 3, H, W, dtype=torch.float64)
    gfeat = torch.randn(graph.dims(B, H, W)[graph.feat], dtype=torch.float64)
    act, g, grads = _autograd_step(graph, sd, img, gfeat)
    return graph, sd, img, gfeat, act, g, grads


def test_graph_shapes_match_autograd(setup):
    graph, sd, img, gfeat, act, g, grads = setup
    dims = graph.dims(B, H, W)
    assert len(dims) == graph.n_nodes == len(act)
    for n in range(graph.n_nodes):
        assert tuple(act[n].shape) == dims[n], n
    cons = graph.consumers
    assert all(cons[n] for n in range(graph.n_nodes) if n != graph.feat) and not cons[graph.feat]
    assert len(graph.pools) == 4 and len(graph.deconvs) == 6 and len(graph.recs) == 48 and graph.n_nodes == 59


def test_reference_reproduces_autograd(setup):
    graph, sd, img, gfeat, act, g, grads = setup
    R = backward_reference(graph, act, g, img, sd, yardstick=False)
    errs = compare_normwise(R, g, grads)
    # every backbone / neck parameter gradient is among the compared quantities
    compared = {n + ".weight" for n in R.dW} | {n + ".weight" for n in R.dWup}
    compared |= {_bn_of(n) + s for n in R.bn for s in (".weight", ".bias")}
    feat_bn = _bn_of(graph.recs[-1][0])
    assert set(grads) - compared == {feat_bn + ".weight", feat_bn + ".bias"}      # (feat's dZ comes from the head backward)
    worst = max(errs, key=errs.get)
    print("\n[backward reference] %d quantities, worst %.3g at %s" % (len(errs), errs[worst], worst))
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad


def _flagged(errs):
    return {k for k, v in errs.items() if not v <= TOL}


def test_control_dropped_residual_share_is_flagged(setup):
    """the residual of level3.tree1.tree2.conv2 detached: its input node (tree1.conv2's output) misses one share"""
    graph, sd, img, gfeat, *_ = setup
    victim = "backbone.level3.tree1.tree2.conv2"
    rec = next(r for r in graph.recs if r[0] == victim)
    owner = next(r[0] for r in graph.recs if r[4] == rec[2])
    act, g, grads = _autograd_step(graph, sd, img, gfeat, drop_res=victim)
    bad = _flagged(compare_normwise(backward_reference(graph, act, g, img, sd, yardstick=False), g, grads))
    assert ("dY", owner) in bad and ("dbeta", owner) in bad, bad
    # nothing downstream of the victim (nearer to `feat`) is touched: those layers' buffers are self-consistent
    later = {r[0] for r in graph.recs if r[4] > rec[2]}
    assert not {k for k in bad if k[1] in later}, bad


def test_control_rolled_deconv_gradient_is_flagged(setup):
    """the gradient of one deconv's output rolled by one column"""
    graph, sd, img, gfeat, act, g, grads = setup
    name, i, o = graph.deconvs[2]
    g2 = dict(g)
    g2[o] = torch.roll(g[o], 1, dims=3)
    bad = _flagged(compare_normwise(backward_reference(graph, act, g2, img, sd, yardstick=False), g2, grads))
    proj = next(r[0] for r in graph.recs if r[4] == i)
    assert {("dZ", name), ("dWup", name), ("dY", proj)} <= bad, bad
    assert all(k[1] in (name, proj) for k in bad), bad


def test_control_swapped_root_sources_are_flagged(setup):
    """the first two source slices of a root conv swapped in the checker's graph: wrong channel offsets"""
    graph, sd, img, gfeat, act, g, grads = setup
    victim = "backbone.level4.tree1.root.conv"
    G2 = PlanGraph()
    G2.__dict__.update(graph.__dict__)
    swap = lambda r: (r[0], [r[1][1], r[1][0]] + r[1][2:], *r[2:]) if r[0] == victim else r      # noqa: E731
    G2.recs = [swap(r) for r in graph.recs]
    G2.steps = [("conv", swap(s[1])) if s[0] == "conv" else s for s in graph.steps]
    rec = next(r for r in graph.recs if r[0] == victim)
    bad = _flagged(compare_normwise(backward_reference(G2, act, g, img, sd, yardstick=False), g, grads))
    owners = {r[0] for r in graph.recs if r[4] in rec[1][:2]}
    assert ("dW", victim) in bad and {("dY", o) for o in owners} <= bad, bad


# ------------------------------------------------------------------------------------------------ the GPU test's own machinery
def _fake_step(setup, g=None, precision="f16x2", stressed=True):
    """the autograd buffers rounded to float32, dressed as a step of test_hip_backward_layers (no GPU): the four partial
    sources are dealt out in turn, so every chain-length formula runs"""
    import test_hip_backward_layers as L
    graph, sd, img, gfeat, act, g0, grads = setup
    g = g0 if g is None else g
    S = L.Step()
    S.cfg, S.shape, S.precision, S.stressed, S.dims_in = "X", "cpu", precision, stressed, (B, H, W)
    S.graph = graph
    S.act = {n: a.float() for n, a in act.items()}
    S.g = {n: a.float() for n, a in g.items()}
    S.grads = {k: v.float() for k, v in grads.items()}
    S.sd = {k: v.float() for k, v in sd.items()}
    S.img = img.float()
    kinds = ("reduce", "twin", "pool", "deconv")
    S.path = {_bn_of(n): kinds[i % 4] for i, n in enumerate([STEM] + [r[0] for r in graph.recs])}
    S.stem_holds = "dY"
    S.R = backward_reference(graph, S.act, S.g, S.img, S.sd, yardstick=True)
    L._evaluate(S)
    return S


def _over(S):
    return ([(k, r[0]) for k, rows in S.conv.items() for r in rows if not r[3] <= 1.0] +
            [(k, r[0]) for k, rows in S.ratio.items() for r in rows if not r[1] <= 1.0])


@pytest.fixture(scope="module")
def fake_step(setup):
    return _fake_step(setup)


def test_yardstick_and_gates_on_autograd_buffers(setup, fake_step):
    """the float32 yard-stick of every conv quantity on buffers that are right to float32 rounding: its error is positive and
    below n * 2^-24 for the longest sum (n <= 2^13 terms here), and every gate of the GPU test holds"""
    graph = setup[0]
    R = fake_step.R
    triples = list(R.dW.items()) + list(R.dWup.items()) + [(n, t) for n, t in R.dZ.items() if n != graph.feat]
    assert len(triples) == 49 + 6 + 58
    for name, t in triples:
        e = t.f32_err()
        assert 0.0 < e < 2.0 ** -11, (name, e)
        assert t.f32.dtype == torch.float32 and t.f32.shape == t.ref.shape == t.mag.shape
    assert set(fake_step.yard) == {"3x3s1", "3x3s2", "1x1", "stem", "deconv", "pool/deconv sums", "conv-node sums"}
    assert not _over(fake_step), _over(fake_step)


def test_gates_flag_a_wrong_buffer(setup):
    """the GPU test's gates on a buffer that is wrong by 2^-12: one pool node's gradient scaled"""
    graph, sd, img, gfeat, act, g, grads = setup
    i, o = graph.pools[1]
    g2 = dict(g)
    g2[o] = g[o] * (1 + 2.0 ** -12)
    over = _over(_fake_step(setup, g=g2, precision="fp32", stressed=False))
    assert ("pool/deconv sums", "pool node %d" % o) in over, over


def test_chain_lengths():
    import test_hip_backward_layers as L
    assert L._chain_length("reduce", 64, 24, 40, 3) == 257
    assert L._chain_length("twin", 64, 24, 40, 3) == 40 and L._chain_length("twin", 512, 3, 5, 3) == 32
    assert L._chain_length("pool", 32, 48, 80, 3) == 4 + 32          # 23 040 quads: one grid-stride iteration, 32 threads per quad
    assert L._chain_length("pool", 64, 192, 640, 32) == 4 * 4 + 16   # 15.7 M quads over 16 384 workgroups of 256
    assert L._chain_length("deconv", 256, 6, 10, 3) == 3 + 10 and L._chain_length("deconv", 64, 12, 156, 2) == 10 + 10


def test_stderr_lines_sees_file_descriptor_2():
    import os
    import test_hip_backward_layers as L
    with L.stderr_lines() as lines:
        os.write(2, b"[plan] from the library\nsecond\n")
    assert lines == ["[plan] from the library", "second"]
