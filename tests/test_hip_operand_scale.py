"""The operand scale of the fp16-split mode (f16x2) on states where it is hard to get right.

f16x2 splits every fp32 operand into two fp16 pieces of x * 2^e, with ONE exponent per tensor.  Two paths take e from a
bound of max |x| instead of the exact value: the lazy (never stored) post-BatchNorm activations, and the stem weight
gradient, which forms its dY operand on the fly.  A bound 2^L too high costs L of the split's 22 bits.  The synthetic
state of the other tests has channels that all look alike, where any bound is close; trained networks do not: train-mode
BatchNorm makes a network invariant to a per-channel rescale of the conv in front of it, and gammas / betas spread over
decades.  `stressed_state_dict` builds such a state from the golden one, and each test compares a layer's output with
an fp64 recomputation from the same inputs, layer by layer (whole-network results would drown in ReLU / max-pool
decision flips).
"""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "monocon-pytorch_amd")
for _p in (PKG, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from plan_graph import (_bn_of, _model, _plan_graph, _read_node, stressed_batch,  # noqa: E402
                        stressed_state_dict)

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
# per-layer error floor in the units of _layer_errors (|gamma_c| + |beta_c|): the fp32 round-off of conv + train-mode
# BatchNorm on these states -- native fp32 mode measures 2e-6 .. 2e-5 per layer, stored f16x2 the same
FLOOR = 2.0 ** -18
SHAPES = [(2, 128, 224), (2, 96, 1248)]      # 1248: KITTI's width, the odd-tile paths of the 16-column kernels
SHAPE_IDS = ["B2_128x224", "B2_96x1248"]


# ------------------------------------------------------------------------------------------------ running a plan
def _forward_nodes(sd, batch, precision, env, monkeypatch, backward=False):
    """one train step's forward (and optionally backward) under `env`; every node's value"""
    for k in ("MONOCON_HIP_LAZY_Z", "MONOCON_HIP_LAZY_MIN", "MONOCON_HIP_LAZY_FEAT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                      # read when the train plan is built
    m = _model(sd, precision)
    gb = {"img": batch["img"].cuda(), "label": {k: v.cuda() for k, v in batch["label"].items()},
          "img_metas": batch["img_metas"]}
    _, loss = m(gb)
    if backward:
        sum(loss.values()).backward()
    torch.cuda.synchronize()
    recs, n_nodes = _plan_graph()
    vals = [_read_node(m, i) for i in range(n_nodes)]
    del m
    torch.cuda.empty_cache()
    return vals


def _layer_errors(sd, vals, with_bound=False, loose=None):
    """per conv layer: its output node against an fp64 recomputation (conv, train-mode BatchNorm, residual, ReLU) from the
    plan's own input nodes.  Error = max over channels of max |err| / (|gamma_c| + |beta_c|) (the size of the channel's
    pre-activation); with_bound: also the f16x2 operand-split bound of each channel, in the same units; loose (a dict): the
    log2 of how far bn_finalize's tensor-wide bound of max |z| lies above the true maximum, per lazy-eligible map."""
    loose = {} if loose is None else loose
    recs, _ = _plan_graph()
    out = {}
    for name, srcs, res, relu, o, ks, stride in recs:
        x = torch.cat([vals[s].double() for s in srcs], 1)
        w = sd[name + ".weight"].double()
        bn = _bn_of(name)
        gamma, beta = sd[bn + ".weight"].double(), sd[bn + ".bias"].double()
        y = F.conv2d(x, w, stride=stride, padding=ks // 2)
        mean = y.mean((0, 2, 3))
        var = y.var((0, 2, 3), unbiased=False)
        a = gamma / torch.sqrt(var + 1e-5)
        z = (y - mean[None, :, None, None]) * a[None, :, None, None] + beta[None, :, None, None]
        if res >= 0:
            z = z + vals[res].double()
        if relu:
            z = z.clamp_min(0)
        got = vals[o].double()
        assert got.shape == z.shape, (name, got.shape, z.shape)
        if res < 0:                     # a lazy-eligible map: bn_finalize's bound of max |z| against the true maximum
            b0 = beta - mean * a
            bound = float((a.abs() * y.abs().max() + (b0 if relu else b0.abs())).clamp_min(0).max())
            loose[name] = math.log2(max(bound, 1e-30) / max(float(z.abs().max()), 1e-30))
        scale = gamma.abs() + beta.abs()
        e_c = (got - z).abs().amax((0, 2, 3))
        err = float((e_c / scale).max())
        if with_bound:
            # |dy_c| <= 2^-21 * sum_s max|x_s| * sum |w_c, s| (each split operand keeps 22 bits of its tensor's max), times
            # |a_c| through the BatchNorm, plus the fp32 rounding of the BatchNorm / residual arithmetic
            terms = torch.zeros_like(gamma)
            c0 = 0
            for s in srcs:
                cs = vals[s].shape[1]
                terms += float(vals[s].abs().max()) * w[:, c0:c0 + cs].abs().sum((1, 2, 3))
                c0 += cs
            zmax_c = z.abs().amax((0, 2, 3))
            bound_c = 2.0 ** -21 * terms * a.abs() + 8 * ULP * (zmax_c + beta.abs() + (mean * a).abs())
            out[name] = (err, float((e_c / bound_c).max()))
        else:
            out[name] = err
    return out


# ------------------------------------------------------------------------------------------------ 1. lazy activations
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_lazy_consumers_match_the_stored_ones_per_layer(golden_sd, shape, monkeypatch):
    """f16x2 with every eligible activation stored (MONOCON_HIP_LAZY_Z=0) against every eligible activation lazy
    (LAZY_Z=3, LAZY_MIN=0) on the stressed state: each conv layer's output against fp64 from its own plan's inputs.  The
    lazy consumers take their operand scale from bn_finalize's bound of max |z|, which on this state lies up to 2^L
    above the true maximum (L is printed) (one tensor-wide max |y| against per-channel BatchNorm multipliers), so the two plans are not
    bit-identical.  What the bound costs must stay below the fp32 round-off of the layer: lazy <= 2 x stored + FLOOR.
    Measured: the worst layer 6.9e-6 lazy against 3.2e-6 stored (level4.tree1.root at 128x224), the rest within 1.8x."""
    B, H, W = shape
    sd = stressed_state_dict(golden_sd)
    batch = stressed_batch(4100 + W, B, H, W)
    stored = _forward_nodes(sd, batch, "f16x2", {"MONOCON_HIP_LAZY_Z": "0"}, monkeypatch)
    lazy = _forward_nodes(sd, batch, "f16x2", {"MONOCON_HIP_LAZY_Z": "3", "MONOCON_HIP_LAZY_MIN": "0"}, monkeypatch)
    e_st = _layer_errors(sd, stored)
    loose = {}
    e_lz = _layer_errors(sd, lazy, loose=loose)
    worse = ["%s: lazy %.3g stored %.3g" % (n, e_lz[n], e_st[n]) for n in e_st if e_lz[n] > 2 * e_st[n] + FLOOR]
    print("\n[operand scale] %s per-layer error (max over channels, |gamma|+|beta| units): " % (shape,) +
          ", ".join("%s %.3g/%.3g" % (n.replace("backbone.", "").replace("neck.", ""), e_st[n], e_lz[n]) for n in e_st))
    worst_l = max(loose, key=loose.get)
    print("[operand scale] bound of max |z| above the true maximum: up to 2^%.1f (%s), median 2^%.1f"
          % (loose[worst_l], worst_l, sorted(loose.values())[len(loose) // 2]))
    assert not worse, "lazy consumers worse than stored ones:\n" + "\n".join(worse)
    assert torch.equal(stored[0], lazy[0])          # the stem: the same kernel and coefficients in both plans


# ------------------------------------------------------------------------------------------------ 2. stem weight gradient
def _stem_step(sd, batch):
    m = _model(sd, "f16x2")
    gb = {"img": batch["img"].cuda(), "label": {k: v.cuda() for k, v in batch["label"].items()},
          "img_metas": batch["img_metas"]}
    _, loss = m(gb)
    sum(loss.values()).backward()
    torch.cuda.synchronize()
    res = {"z0": _read_node(m, 0), "g0": _read_node(m, 0, 1), "g1": _read_node(m, 1, 1),
           "dw": m.state_dict(keep_vars=True)["backbone.base_layer.0.weight"].grad.detach().cpu().clone()}
    del m
    torch.cuda.empty_cache()
    return res


def _stem_inputs(golden_sd, H, W):
    return stressed_state_dict(golden_sd), stressed_batch(4200 + W, 2, H, W)


@pytest.mark.parametrize("shape", [(128, 224), (96, 1248)], ids=["128x224", "96x1248"])
def test_fused_stem_weight_gradient_matches_the_unfused_one(golden_sd, shape, monkeypatch):
    """the stem weight gradient with dY formed on the fly from (d, y, BatchNorm coefficients) and scaled by a bound
    (MONOCON_HIP_STEM_FUSE, the default) against the separate element-wise pass (STEM_FUSE=0, read when the train plan
    is built: a second model in this process), both against fp64 conv2d_weight(img, dY) with dY the fp64 BatchNorm
    backward of the stem node's gradient (the GPU's own ReLU mask: no decision flips).  Everything upstream of the stem
    is the same computation."""
    H, W = shape
    monkeypatch.setenv("MONOCON_HIP_GRAD_POOL", "0")                 # private gradient buffers: readable after the step
    monkeypatch.delenv("MONOCON_HIP_STEM_FUSE", raising=False)
    sd, batch = _stem_inputs(golden_sd, H, W)
    fus = _stem_step(sd, batch)
    monkeypatch.setenv("MONOCON_HIP_STEM_FUSE", "0")
    unf = _stem_step(sd, batch)
    assert torch.equal(fus["g1"], unf["g1"])          # level0's gradient: upstream of the stem's weight gradient, bit-equal
    assert torch.equal(fus["z0"], unf["z0"])
    # the stem node's gradient buffer: dZ in the fused run; the separate pass overwrites it with dY in place
    img = batch["img"].double()
    w = sd["backbone.base_layer.0.weight"].double()
    gamma = sd["backbone.base_layer.1.weight"].double()
    y = F.conv2d(img, w, padding=3)
    mean = y.mean((0, 2, 3), keepdim=True)
    var = y.var((0, 2, 3), unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    yhat = (y - mean) * rstd
    d = fus["g0"].double() * (fus["z0"] > 0).double()          # the GPU's own ReLU mask
    dy = gamma[None, :, None, None] * rstd * (d - d.mean((0, 2, 3), keepdim=True) - yhat * (d * yhat).mean((0, 2, 3), keepdim=True))
    # (channels that the ReLU kills everywhere -- beta < 0 on this state -- have dY = 0: a floor at 1e-3 of the largest)
    m_dy = dy.abs().amax((0, 2, 3))
    e_dy = (unf["g0"].double() - dy).abs().amax((0, 2, 3)) / m_dy.clamp_min(1e-3 * float(m_dy.max()))
    assert float(e_dy.max()) < 1e-3, e_dy                      # (what the unfused weight gradient read)
    dw = torch.nn.grad.conv2d_weight(img, w.shape, dy, padding=3)
    scale = dw.abs().amax((1, 2, 3))
    scale = scale.clamp_min(1e-3 * float(scale.max()))

    def err(g):
        return float(((g.double() - dw).abs().amax((1, 2, 3)) / scale).max())

    e_f, e_u = err(fus["dw"]), err(unf["dw"])
    print("\n[operand scale] stem weight gradient %dx%d: fused %.3g, unfused %.3g (max over channels, relative)" % (H, W, e_f, e_u))
    assert e_f <= 2 * e_u + 4 * ULP, (e_f, e_u)


# ------------------------------------------------------------------------------------------------ 3. the per-tensor scale
@pytest.mark.parametrize("shape", SHAPES[:1], ids=SHAPE_IDS[:1])
def test_stored_f16x2_layers_keep_22_bits_of_the_operand_maximum(golden_sd, shape, monkeypatch):
    """stored-mode f16x2 against native fp32 per layer, both against fp64 from their own inputs, on the stressed state.
    The design's promise for the split with one exponent per tensor: |err| <= 2^-21 * max|operand| * sum|w| per output
    (through the BatchNorm: times |a_c|), plus fp32 rounding."""
    B, H, W = shape
    sd = stressed_state_dict(golden_sd)
    batch = stressed_batch(4300 + W, B, H, W)
    f16 = _layer_errors(sd, _forward_nodes(sd, batch, "f16x2", {"MONOCON_HIP_LAZY_Z": "0"}, monkeypatch), with_bound=True)
    f32 = _layer_errors(sd, _forward_nodes(sd, batch, "fp32", {}, monkeypatch))
    ratios = sorted(f16[n][0] / max(f32[n], 1e-30) for n in f16)
    print("\n[operand scale] f16x2 (stored) / fp32 per-layer error ratio: median %.3g, max %.3g; worst error / bound %.3g"
          % (ratios[len(ratios) // 2], ratios[-1], max(v[1] for v in f16.values())))
    over = ["%s: %.3g of the bound" % (n, v[1]) for n, v in f16.items() if v[1] > 1.0]
    assert not over, "\n".join(over)

