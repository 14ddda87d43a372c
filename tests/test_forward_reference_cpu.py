"""The layer-local forward reference of `plan_graph.py` and the gates of test_hip_forward_layers.py, checked without a GPU.

The oracle's train forward (`oracle.monocon_oracle`: `backbone` and `neck` as `train_forward` runs them, with a `_Ctx` that
also records what every conv reads and every BatchNorm returns) runs at 2x64x96 on the golden state.  What its convs read ARE the graph's nodes: a node
with several consumers must arrive bit-equal at each of them, which proves the graph's source lists against the oracle.  The
activations go to `forward_reference` as `act`:

  in float64, every node and every running buffer must reproduce at float64 round-off (1e-12 norm-wise);
  in float32, the gates of the GPU test must pass with the oracle as "the GPU";
  eleven negative controls, applied to those float32 buffers, must each be flagged by the gate they belong to.  2x64x96 gives
  1x1 ... 2x3 maps at level5 (n = 12): the n / (n - 1) factor is 9 %.
"""
import pytest
import torch
import torch.nn.functional as F

from plan_graph import (BN_MOMENTUM, EPS, STEM, STEM_REC, PlanGraph, _bn_of, _plan_convs, forward_reference, norm_err, plan_graph)

B, H, W = 2, 64, 96
TOL = 1e-12
U = 2.0 ** -24


def oracle_forward(sd, img):
    """the oracle's train forward of backbone + neck: ({node: activation}, new running buffers, what the dead projects read)"""
    from oracle import monocon_oracle as O

    class Recorder(O._Ctx):
        def __init__(self, sd):
            super().__init__(sd, True)
            self.conv_in, self.bn_out = {}, {}

        def conv(self, x, name, stride=1, pad=0):
            self.conv_in[name] = x
            return super().conv(x, name, stride, pad)

        def bn(self, x, name, *args, **kw):
            self.bn_out[name] = super().bn(x, name, *args, **kw)
            return self.bn_out[name]

    cx = Recorder(sd)
    with torch.no_grad():
        feat = O.neck(cx, O.backbone(cx, img))
    G = plan_graph()
    act = {G.feat: feat}
    for name, srcs, res, relu, o, ks, stride in G.recs:
        c0 = 0
        for s in srcs:
            x = cx.conv_in[name][:, c0:c0 + G.node_c[s]]
            c0 += G.node_c[s]
            assert s not in act or torch.equal(act[s], x), (name, s)          # one node, whoever reads it
            act[s] = x
        assert c0 == cx.conv_in[name].shape[1]
    # nodes no conv reads -- a `project` (read as a residual) and the neck's proj (read by its deconv): the BatchNorm's output,
    # through the ReLU where the layer has one
    for name, srcs, res, relu, o, ks, stride in G.recs:
        if o not in act:
            assert res < 0 and (name.endswith(".project.0") or ".proj_" in name), name
            act[o] = F.relu(cx.bn_out[_bn_of(name)]) if relu else cx.bn_out[_bn_of(name)]
    assert torch.equal(cx.conv_in[STEM], img)
    for name, src in G.dead:
        assert torch.equal(cx.conv_in[name], act[src]), name
    assert set(act) == set(range(G.n_nodes))
    return act, cx.new_buffers


@pytest.fixture(scope="module")
def oracle32(golden_sd):
    from hipmonocon import synth
    batch = synth.make_batch(6100, B, H, W)
    act, newbuf = oracle_forward(golden_sd, batch["img"])
    return batch, act, newbuf


def test_recorded_forward_is_the_oracles_train_forward(golden_sd, oracle32):
    """the recording context changes nothing: `train_forward` leaves the same running buffers, bit for bit, and the graph's
    dead list names exactly the BatchNorms of `_plan_convs()` that no record covers"""
    from oracle import monocon_oracle as O
    batch, act, newbuf = oracle32
    with torch.no_grad():
        _, _, _, ref = O.train_forward(golden_sd, batch)
    ours = {k: v for k, v in ref.items() if k.startswith("backbone.") or k.startswith("neck.")}
    assert set(ours) == set(newbuf) and all(torch.equal(ours[k], newbuf[k]) for k in ours)
    G = plan_graph()
    assert [n for n, _ in G.dead] == ["backbone.level3.project.0", "backbone.level4.project.0"]
    assert {n for n, _ in _plan_convs()} == {STEM} | {r[0] for r in G.recs} | {n for n, _ in G.dead}
    assert {bn + s for _, bn in _plan_convs() for s in (".running_mean", ".running_var", ".num_batches_tracked")} == set(newbuf)
    pool_of = {o: i for i, o in G.pools}
    assert all(src in pool_of for _, src in G.dead)          # their input is the `bottom` pool node


def test_reference_reproduces_the_oracle_in_float64(golden_sd, oracle32):
    batch = oracle32[0]
    sd64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in golden_sd.items()}
    img = batch["img"].double()
    act, newbuf = oracle_forward(sd64, img)
    G = plan_graph()
    R = forward_reference(G, act, img, sd64, yardstick=False)
    errs = {}
    for kind, name, o, t in R.layers:
        errs[("z", name)] = norm_err(act[o], t.ref)
        assert bool((t.mag >= t.ref.abs() * (1 - 1e-12)).all()), name          # a magnitude sum bounds its value
    for name, i, o, t in R.deconvs:
        errs[("deconv", name)] = norm_err(act[o], t.ref)
    for i, o, want in R.pools:
        assert torch.equal(act[o], want) and torch.equal(want, F.max_pool2d(act[i], 2, 2)), (i, o)
    assert len(R.layers) == 49 and len(R.deconvs) == 6 and len(R.pools) == 4 and len(R.running) == 51
    for bn, run in R.running.items():
        errs[("running_mean", bn)] = norm_err(newbuf[bn + ".running_mean"], run["rm"].ref)
        errs[("running_var", bn)] = norm_err(newbuf[bn + ".running_var"], run["rv"].ref)
        assert int(newbuf[bn + ".num_batches_tracked"]) == run["nbt"] == 1
    worst = max(errs, key=errs.get)
    print("\n[forward reference] %d quantities, worst %.3g at %s" % (len(errs), errs[worst], worst))
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    # the statistics the bounds are made of
    st = R.stats["backbone.level5.tree1.conv1"]
    assert st["n"] == 12 and st["K"] == 256 * 9
    assert torch.allclose(st["e2"], st["var"] + st["m0"] ** 2, rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------------------------ the GPU test's own machinery
PRODUCERS = ("fp32", "row", "chan_reduce", "split", "stem_f16", "wres", "thin16", "fp32_ws", "row_lazy")


def _fake_step(golden_sd, oracle32, act=None, after=None, graph=None, precision="fp32", lazy=()):
    """the oracle's float32 buffers dressed as a forward of test_hip_forward_layers (no GPU): the statistics producers are
    dealt out in turn, so every chain-length formula runs; act / after: buffers a control has tampered with; lazy: nodes
    the plan lines report as never stored"""
    import test_hip_forward_layers as L
    batch, act0, newbuf = oracle32
    S = L.Step()
    S.cfg, S.shape, S.precision, S.dims_in = "X", "cpu", precision, (B, H, W)
    S.graph = G = plan_graph() if graph is None else graph
    S.act = dict(act0) if act is None else act
    S.img = batch["img"]
    S.sd_before = golden_sd
    S.sd_after = dict(golden_sd)
    S.sd_after.update(newbuf)
    S.sd_after.update(after or {})
    node_of = {_bn_of(STEM): 0}
    node_of.update({_bn_of(r[0]): r[4] for r in G.recs})
    S.producer = {bn: (node_of.get(bn, -1), PRODUCERS[i % len(PRODUCERS)], 100, "float",
                       ("lazy" if node_of[bn] in lazy else "stored") if bn in node_of else "dead")
                  for i, (_, bn) in enumerate(_plan_convs())}
    S.materialised = set()
    S.R = forward_reference(S.graph, S.act, S.img, S.sd_before, yardstick=True)
    L._evaluate(S)
    return S


def _over(S):
    """(class, label) of everything that missed its gate; statistics labels lose their '(producer, finalize)' suffix"""
    out = [(k, r[0]) for k, rows in S.conv.items() for r in rows if not r[3] <= 1.0]
    out += [(k, r[0].split(" (")[0]) for k, rows in S.ratio.items() for r in rows if not r[1] <= 1.0]
    out += [("pools", l) for l in S.bad_pools] + [("nbt", l.split(".num_batches_tracked")[0]) for l in S.bad_nbt]
    return out


@pytest.fixture(scope="module")
def fake_step(golden_sd, oracle32):
    return _fake_step(golden_sd, oracle32)


def test_gates_pass_with_the_oracle_as_the_gpu(fake_step):
    """torch's float32 forward is right to float32 rounding: every gate of the GPU test holds, the float32 yard-stick of every
    kind is positive and small, and everything the coverage test counts was counted"""
    S = fake_step
    assert not _over(S), _over(S)
    assert set(S.yard) == {"stem", "3x3s1", "3x3s2", "1x1", "deconv"}
    for kind, y in S.yard.items():
        assert 0.0 < y < 2.0 ** -18, (kind, y)
    assert set(S.ratio) == {"batch mean", "batch var", "running_mean", "running_var"}
    assert all(len(rows) == 51 for rows in S.ratio.values())
    assert S.checked["nodes"] == set(range(S.graph.n_nodes)) and {q[1] for q in S.producer.values()} == set(PRODUCERS)
    assert S.checked["consumers"] == {(k, "stored") for k in ("conv", "pool", "deconv")}
    worst = {c: max(r[1] for r in rows) for c, rows in S.ratio.items()}
    print("\n[forward reference] oracle float32 as the GPU: worst measured / bound %s; conv worst of the gate %.3g"
          % (worst, max(r[3] for rows in S.conv.values() for r in rows)))


def _rec(G, name):
    return STEM_REC if name == STEM else next(r for r in G.recs if r[0] == name)


def _layer(golden_sd, oracle32, name, var_of=None, eps=EPS, res=True, relu=None, srcs=None, mean_of=None):
    """node `name` as a defective kernel would leave it: float64 from the oracle's float32 inputs, rounded to float32"""
    G = plan_graph()
    batch, act, _ = oracle32
    _, s0, r, rl, o, ks, stride = _rec(G, name)
    xs = [batch["img"]] if name == STEM else [act[s] for s in (s0 if srcs is None else srcs)]
    y = F.conv2d(torch.cat([t.double() for t in xs], 1), golden_sd[name + ".weight"].double(), stride=stride, padding=ks // 2)
    bn = _bn_of(name)
    n = y.numel() // y.shape[1]
    mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    if var_of is not None:
        var = var_of(var, n)
    if mean_of is not None:
        mean = mean_of(mean)
    a = golden_sd[bn + ".weight"].double() / torch.sqrt(var + eps)
    z = (y - mean[None, :, None, None]) * a[None, :, None, None] + golden_sd[bn + ".bias"].double()[None, :, None, None]
    if r >= 0 and res:
        z = z + act[r].double()
    if rl if relu is None else relu:
        z = z.clamp_min(0)
    return o, z.float()


def _with(oracle32, o, z):
    act = dict(oracle32[1])
    act[o] = z
    return act


L5 = "backbone.level5.tree1.conv1"          # 3x3 stride 2 onto the 2x3 maps: n = 12


def test_control_unbiased_variance_in_a(golden_sd, oracle32):
    o, z = _layer(golden_sd, oracle32, L5, var_of=lambda var, n: var * n / (n - 1))
    assert ("3x3s2", L5) in _over(_fake_step(golden_sd, oracle32, act=_with(oracle32, o, z)))


def test_control_biased_variance_in_running_var(golden_sd, oracle32):
    bn = _bn_of(L5)
    S0 = _fake_step(golden_sd, oracle32)
    st = S0.R.stats[L5]
    assert st["n"] == 12
    m = BN_MOMENTUM
    rv = ((1 - m) * golden_sd[bn + ".running_var"].double() + m * st["var"]).float()
    over = _over(_fake_step(golden_sd, oracle32, after={bn + ".running_var": rv}))
    assert ("running_var", bn) in over and ("batch var", bn) in over, over
    assert not [k for k in over if k[1] != bn], over


def test_control_momentum(golden_sd, oracle32):
    """momentum 0.9 instead of 0.1, on the stem: visible where the batch statistic differs from the running one"""
    bn = _bn_of(STEM)
    st = _fake_step(golden_sd, oracle32).R.stats[STEM]
    n = st["n"]
    rm = (0.1 * golden_sd[bn + ".running_mean"].double() + 0.9 * st["mean"]).float()
    rv = (0.1 * golden_sd[bn + ".running_var"].double() + 0.9 * st["var"] * n / (n - 1)).float()
    over = _over(_fake_step(golden_sd, oracle32, after={bn + ".running_mean": rm, bn + ".running_var": rv}))
    assert {("running_mean", bn), ("running_var", bn), ("batch mean", bn), ("batch var", bn)} <= set(over), over


def test_control_eps(golden_sd, oracle32):
    """eps 1e-3 instead of 1e-5 in a: applied where the batch variance is smallest (it is visible where var is not >> 1e-3)"""
    R = _fake_step(golden_sd, oracle32).R
    G = plan_graph()
    name = min((r[0] for r in G.recs), key=lambda nm: float(R.stats[nm]["var"].min()))
    assert float(R.stats[name]["var"].min()) < 1.0, (name, float(R.stats[name]["var"].min()))
    o, z = _layer(golden_sd, oracle32, name, eps=1e-3)
    kind = next(k for k, nm, _, _ in R.layers if nm == name)
    assert (kind, name) in _over(_fake_step(golden_sd, oracle32, act=_with(oracle32, o, z)))


def test_control_residual_left_out(golden_sd, oracle32):
    name = "backbone.level3.tree1.tree2.conv2"
    o, z = _layer(golden_sd, oracle32, name, res=False)
    assert ("3x3s1", name) in _over(_fake_step(golden_sd, oracle32, act=_with(oracle32, o, z)))


def test_control_relu_on_a_project(golden_sd, oracle32):
    name = "backbone.level2.project.0"
    o, z = _layer(golden_sd, oracle32, name, relu=True)
    assert not _rec(plan_graph(), name)[3] and bool((oracle32[1][o] < 0).any())
    assert ("1x1", name) in _over(_fake_step(golden_sd, oracle32, act=_with(oracle32, o, z)))


def test_control_swapped_root_sources(golden_sd, oracle32):
    name = "backbone.level4.tree1.root.conv"
    srcs = _rec(plan_graph(), name)[1]
    o, z = _layer(golden_sd, oracle32, name, srcs=[srcs[1], srcs[0]] + srcs[2:])
    over = _over(_fake_step(golden_sd, oracle32, act=_with(oracle32, o, z)))
    assert ("1x1", name) in over, over
    # the same defect in the checker's graph instead: flagged at the same layer, and in its statistics
    G = plan_graph()
    G2 = PlanGraph()
    G2.__dict__.update(G.__dict__)
    swap = lambda r: (r[0], [r[1][1], r[1][0]] + r[1][2:], *r[2:]) if r[0] == name else r      # noqa: E731
    G2.recs = [swap(r) for r in G.recs]
    G2.steps = [("conv", swap(s[1])) if s[0] == "conv" else s for s in G.steps]
    over = _over(_fake_step(golden_sd, oracle32, graph=G2))
    assert ("1x1", name) in over and ("batch var", _bn_of(name)) in over, over


def test_control_rolled_deconv(golden_sd, oracle32):
    name, i, o = plan_graph().deconvs[2]
    over = _over(_fake_step(golden_sd, oracle32, act=_with(oracle32, o, torch.roll(oracle32[1][o], 1, dims=3))))
    assert ("deconv", name) in over, over


def test_control_pool_of_a_lazy_map(golden_sd, oracle32):
    """a pool whose input the plan reports lazy is held to 4 U of the pooled |a| |y64| + |b|: the exact pool passes (0 of the
    bound), one off by 16 U is flagged -- where y and b have one sign that magnitude IS |z|, so 16 U |z| exceeds it"""
    i, o = plan_graph().pools[0]
    S = _fake_step(golden_sd, oracle32, lazy={i})
    assert S.ratio["lazy pools"] == [("pool node %d of lazy node %d" % (o, i), 0.0)] and not _over(S)
    assert ("pool", "lazy") in S.checked["consumers"] and ("conv", "lazy") in S.checked["consumers"]
    off = (oracle32[1][o].double() * (1 + 16 * U)).float()
    over = _over(_fake_step(golden_sd, oracle32, act=_with(oracle32, o, off), lazy={i}))
    assert ("lazy pools", "pool node %d of lazy node %d" % (o, i)) in over, over


def test_control_dead_project_left_unticked(golden_sd, oracle32):
    name = plan_graph().dead[1][0]
    bn = _bn_of(name)
    after = {bn + k: golden_sd[bn + k].clone() for k in (".running_mean", ".running_var", ".num_batches_tracked")}
    over = _over(_fake_step(golden_sd, oracle32, after=after))
    assert {("running_mean", bn), ("running_var", bn), ("nbt", bn)} <= set(over), over


def test_control_perturbed_mean(golden_sd, oracle32):
    """one channel's batch mean off by k U |mean|, in the running mean and in b.  An error of 64 U |mean| is below every derived
    bound: dy_c alone is 4 sqrt(K) U max M_y,c >= 4 sqrt(147) U |mean| = 48.5 U |mean|, the chain term adds
    (L + 8) U E|y - shift|, and recovering the mean from the running buffers costs 4 U (|rm'| + |rm|) / m = 76 U |mean| on a
    calibrated state (asserted: k > 64 everywhere).  So the control takes the (layer, channel) where the running-mean
    allowance of `_evaluate` is tightest relative to |mean|, reports how many U |mean| it is worth, and perturbs by twice
    that: flagged there, and only there."""
    S0 = _fake_step(golden_sd, oracle32)
    m = BN_MOMENTUM
    best = None
    for name, bn in _plan_convs():
        st = S0.R.stats[name]
        if st["node"] is None:
            continue
        k = S0.tol[("running_mean", bn)] / (m * U * st["mean"].abs().clamp_min(1e-300))
        c = int(k.argmin())
        if best is None or float(k[c]) < best[0]:
            best = (float(k[c]), name, bn, c)
    k, name, bn, c = best
    assert k > 64, "a 64 U |mean| error is visible after all at %s channel %d (%.3g): use it" % (name, c, k)
    k2 = 2 * k
    print("\n[forward reference] the tightest running-mean bound is worth %.0f U |mean| (%s, channel %d); perturbing by %.0f" % (k, bn, c, k2))

    def off(mean):
        mean = mean.clone()
        mean[c] *= 1 + k2 * U
        return mean

    o, z = _layer(golden_sd, oracle32, name, mean_of=off)
    st = S0.R.stats[name]
    rm = ((1 - m) * golden_sd[bn + ".running_mean"].double() + m * off(st["mean"])).float()
    over = _over(_fake_step(golden_sd, oracle32, act=_with(oracle32, o, z), after={bn + ".running_mean": rm}))
    assert ("running_mean", bn) in over, over
    assert not [x for x in over if x[0] in ("running_mean", "batch mean", "running_var", "batch var") and x[1] != bn], over


def test_chain_lengths():
    import test_hip_forward_layers as L
    assert all(L._chain_length(p, 40) == 32 for p in ("fp32", "fp32_ws", "split", "wres"))          # a 4x8 patch
    assert all(L._chain_length(p, 40) == 40 and L._chain_length(p, 1248) == 1248 for p in ("row", "row_lazy", "thin16", "stem_f16"))
    assert L._chain_length("chan_reduce", 1248) == 257
    with pytest.raises(KeyError):
        L._chain_length("a kernel nobody derived a bound for", 40)


def test_plan_lines_are_parsed():
    import test_hip_forward_layers as L
    prod, mat = L.parse_forward_lines([
        "[plan] forward backbone.base_layer.1                    node   0  statistics by stem_f16      192 partial rows  finalize float  z lazy",
        "[plan] forward backbone.level3.project.1                node  -1  statistics by split          12 partial rows  finalize float  z dead",
        "[plan] forward backbone.level0.1                        node   1  statistics by split        7488 partial rows  finalize double  z stored",
        "[plan] lazy node 7 (64 ch 24x40) materialised for a consumer that cannot form it on load"])
    assert prod == {"backbone.base_layer.1": (0, "stem_f16", 192, "float", "lazy"),
                    "backbone.level3.project.1": (-1, "split", 12, "float", "dead"),
                    "backbone.level0.1": (1, "split", 7488, "double", "stored")}
    assert mat == {7}


def test_fresh_state_resets_every_plan_batchnorm(golden_sd):
    import test_hip_forward_layers as L
    sd = L.fresh_state_dict(golden_sd)
    for _, bn in _plan_convs():
        assert float(sd[bn + ".running_mean"].abs().max()) == 0.0 and bool((sd[bn + ".running_var"] == 1).all())
    assert float(golden_sd["backbone.level0.1.running_var"].sub(1).abs().max()) > 0          # (the golden state is left alone)
