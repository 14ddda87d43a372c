"""The image as a differentiable input of the HIP train step: img.grad through mc_backward_image_grad and the stem's 7x7
data gradient (stem_dgrad_kernel, fp32 in every precision mode).

  1 whole chain     img.grad of the two flip-free fixtures against the reference's fp64 gradient (tests/golden/img_grad.npz),
                    relative L2 <= 1e-3: the gate test_conditioned_gradients_vs_reference_fp64 applies to every parameter
                    tensor of these fixtures.  Measured on an MI355X, worst of the two cases: fp32 8.0e-5, bf16x3 8.0e-5,
                    f16x2 9.2e-6 (the reference's own fp32 run: 1.0e-5): see MEASURED_PARITY.
  2 the kernel      on the plan's own buffers against conv_transpose2d in fp64 (stored and fused form), the conv gate of
                    test_hip_backward_layers: elementwise |got - ref| / M, M the same operation on absolute values floored at
                    2^-10 of its maximum; yard-stick the same transposed conv by torch in float32 from the same buffers; gate
                    HIP <= 5 x yard-stick's worst + 4 U.  Fused form: + 8 U (|P d| + |Q y| + |R|) carried through the
                    transposed conv of |W| (the rounding of the three-term dY that file states).  See MEASURED.
  3 nothing moves   a step that asks for the image gradient and one that does not: bit-identical losses, parameter
                    gradients and running buffers; with the gradient pool, without it, and on one stream.
  4 autograd        weighted objective, non-leaf image, accumulation, heads-only plan, NULL grad_img.
  5 op level        mc_op_stem_dgrad / mc_op_stem_dgrad_fused at ragged shapes against conv2d_input in fp64, gate of 2.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from hipmonocon import synth
from plan_graph import EPS, STEM, _floored, _model, _read_node
from test_hip_backward_layers import stderr_lines
from test_hip_train_step import build, to_cuda

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PRECISIONS = ("fp32", "bf16x3", "f16x2")
SWITCHES = ("LAZY_Z", "LAZY_MIN", "LAZY_FEAT", "ZBITS", "GRAD_POOL", "GRAD_POOL_COOL", "HEAD_DX_FUSE", "DGRAD_S2_THIN", "STEM_FUSE",
            "BM_EPILOGUE", "WRES_BWD", "DUAL_STREAM", "SIDE_SYNC", "PLAN_DEBUG")
# measured on an MI355X: relative L2 of img.grad against the reference's fp64 gradient, worst of cases 0 and 1 (gate 1e-3;
# the reference's own fp32 run: 9.7e-6 / 1.04e-5)
MEASURED_PARITY = """
          case 0    case 1
fp32      1.32e-5   8.00e-5
bf16x3    9.53e-6   7.97e-5
f16x2     9.21e-6   8.24e-6
"""
# measured on an MI355X, worst over the config's shapes: HIP error / float32 yard-stick error (both of the magnitude sum),
# and the worst |got - ref| / gate (gate: 1)
MEASURED = """
config     stem buffer   HIP / float32 yard-stick     of the gate
A fp32     dY            4.97e-7 / 4.06e-7 = 1.22     0.219
G f16x2    dY            4.40e-7 / 4.22e-7 = 1.04     0.187
C f16x2    d (fused)     3.68e-7 / 4.18e-7 = 0.88     0.131
default    d (fused)     4.36e-7 / 4.26e-7 = 1.02     0.153
(default includes 2x96x1248: 4.64e-7 / 5.04e-7 = 0.92, 0.143 of the gate.  Op level, stored / fused: at most 3.12e-7 / 2.62e-7
beside float32's 2.75e-7 / 2.52e-7, 0.193 / 0.120 of the gate.)
"""


def _say(line):
    print("\n[image grad] " + line)


def rel_l2(got, ref):
    return float((got.detach().cpu().double() - ref).norm() / max(float(ref.norm()), 1e-30))


def _clean_env(mp, env=None):
    for k in SWITCHES:
        mp.delenv("MONOCON_HIP_" + k, raising=False)
    for k, v in (env or {}).items():
        mp.setenv(k, v)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ 1: the whole chain
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", [0, 1])
def test_image_gradient_vs_reference_fp64(cond_sd, case, precision):
    """img.grad of sum(loss_dict.values()).backward() against the reference's fp64 gradient of the same fixture, relative L2
    <= 1e-3.  Measured, worst of the two cases: fp32 8.0e-5, bf16x3 8.0e-5, f16x2 9.2e-6 (MEASURED_PARITY); the reference's
    own fp32 run sits at 1.0e-5.  Without the feature img.grad is None."""
    g = load_golden("img_grad.npz")
    B, H, W = (int(x) for x in g["c%d.shape" % case])
    m = build(cond_sd, precision)
    batch = to_cuda(synth.make_conditioned_batch(int(g["c%d.seed" % case]), B, H, W))
    img = batch["img"].requires_grad_()
    _, loss = m(batch)
    sum(loss.values()).backward()
    torch.cuda.synchronize()
    assert img.grad is not None, "the train step left no gradient in the image"
    assert img.grad.shape == img.shape and img.grad.dtype == torch.float32
    ref = torch.from_numpy(g["c%d.g64" % case]).double()
    e = rel_l2(img.grad, ref)
    _say("case %d %-6s img.grad vs fp64 %.3g (reference fp32-vs-fp64 %.3g / %.3g one thread; norm %.4g, reference %.4g)"
         % (case, precision, e, float(g["c%d.gerr32" % case]), float(g["c%d.gerr32_1t" % case]), float(img.grad.double().norm()),
            float(g["c%d.gnorm64" % case])))
    assert e <= 1e-3, e


# ------------------------------------------------------------------------------------------------ 2: the kernel on the plan
def _conv_gate(got, ref, mag, f32, extra=None):
    """(HIP error, yard-stick error, worst |got - ref| / gate) in the terms of test_hip_backward_layers' conv gate"""
    fl = _floored(mag)
    err = (got.double() - ref).abs()
    yard = float(((f32.double() - ref).abs() / fl).max())
    allowed = (5 * yard + 4 * U) * fl
    if extra is not None:
        allowed = allowed + extra
    return float((err / fl).max()), yard, float((err / allowed).max())


def _fused_dy(d, y, gamma):
    """dY = P d + Q y + R of a BatchNorm + ReLU backward in fp64 from the masked gradient d and the raw conv output y (NCHW),
    as plan_graph.backward_reference forms the stem's; also the three terms' magnitudes |P d| + |Q y| + |R|"""
    n = y.numel() // y.shape[1]
    v = lambda t: t[None, :, None, None]          # noqa: E731
    mean = y.mean((0, 2, 3))
    rstd = 1.0 / torch.sqrt(y.var((0, 2, 3), unbiased=False) + EPS)
    yhat = (y - v(mean)) * v(rstd)
    dbeta, dgamma = d.sum((0, 2, 3)), (d * yhat).sum((0, 2, 3))
    a = gamma * rstd
    P, Q, R = a, -a * rstd * dgamma / n, -a * dbeta / n + a * rstd * mean * dgamma / n
    return v(P) * d + v(Q) * y + v(R), v(P.abs()) * d.abs() + v(Q.abs()) * y.abs() + v(R.abs()) * torch.ones_like(y)


LAYER_CONFIGS = {   # precision, switches, what the stem's gradient buffer holds after the backward
    "A": ("fp32", {}, "dY"),
    "G": ("f16x2", {"MONOCON_HIP_STEM_FUSE": "0"}, "dY"),
    "C": ("f16x2", {"MONOCON_HIP_LAZY_Z": "0"}, "d"),
    "default": ("f16x2", {}, "d"),
}
LAYER_SHAPES = {"3x96x160": (3, 96, 160), "2x64x224": (2, 64, 224), "2x96x1248": (2, 96, 1248)}
LAYER_CASES = [(c, s) for c in LAYER_CONFIGS for s in ("3x96x160", "2x64x224")] + [("default", "2x96x1248")]


@pytest.mark.parametrize("cfg,shape", LAYER_CASES, ids=["%s-%s" % cs for cs in LAYER_CASES])
def test_stem_dgrad_on_the_plans_buffers(golden_sd, cfg, shape, monkeypatch):
    """img.grad of one train step against conv_transpose2d in fp64 of the dY the plan's own stem buffer holds (stored form),
    or of the dY formed in fp64 from the masked d it holds, the fp64 raw output and the fp64 statistics (fused form)"""
    precision, env, holds = LAYER_CONFIGS[cfg]
    B, H, W = LAYER_SHAPES[shape]
    _clean_env(monkeypatch, dict(env, MONOCON_HIP_GRAD_POOL="0", MONOCON_HIP_PLAN_DEBUG="1"))
    batch = synth.make_batch(5300 + W, B, H, W)
    with stderr_lines() as err:
        m = _model(golden_sd, precision)
        gb = to_cuda(batch)
        img = gb["img"].requires_grad_()
        _, loss = m(gb)
        sum(loss.values()).backward()
        torch.cuda.synchronize()
    got = img.grad.detach().cpu()
    gbuf, z = _read_node(m, 0, 1).double(), _read_node(m, 0, 0)
    del m
    torch.cuda.empty_cache()
    # which form ran: the plan's own debug lines (the rule of test_hip_backward_layers)
    twin, cur = False, None
    for l in err:
        mm = re.match(r"\[plan\] bn_backward (\S+)", l)
        if mm:
            cur = mm.group(1)
        elif l.startswith("[plan]   twin of") and cur == "backbone.base_layer.1":
            twin = True
    fused = precision == "f16x2" and env.get("MONOCON_HIP_STEM_FUSE", "1") != "0" and twin
    assert ("d" if fused else "dY") == holds, (cfg, fused, twin)
    w = golden_sd[STEM + ".weight"].double()
    extra = None
    if fused:
        assert float((gbuf.abs() * (z <= 0)).max()) == 0.0, "the stem's masked gradient is not zero where z = 0"
        y = F.conv2d(batch["img"].double(), w, padding=3)
        dY, terms = _fused_dy(gbuf, y, golden_sd["backbone.base_layer.1.weight"].double())
        extra = F.conv_transpose2d(8 * U * terms, w.abs(), padding=3)
    else:
        dY = gbuf
    ref = F.conv_transpose2d(dY, w, padding=3)
    mag = F.conv_transpose2d(dY.abs(), w.abs(), padding=3)
    f32 = F.conv_transpose2d(dY.float(), w.float(), padding=3)
    e, yard, of_gate = _conv_gate(got, ref, mag, f32, extra)
    _say("%s %s (%s, buffer holds %s): HIP %.3g / float32 %.3g = %.2f, %.3g of the gate"
         % (cfg, shape, precision, holds, e, yard, e / max(yard, 1e-30), of_gate))
    assert of_gate <= 1.0, (e, yard, of_gate)


# ------------------------------------------------------------------------------------------------ 3: nothing else moves
def _buffers(m):
    return {n: v.detach().clone() for n, v in m.named_buffers()}


def _restore(m, saved):
    """the forward accumulates its batch statistics shifted by the running mean, so two steps are bit-identical only from
    equal running buffers: put back the ones a fresh model had"""
    with torch.no_grad():
        for n, v in m.named_buffers():
            v.copy_(saved[n])


def _step(m, batch, want_img_grad):
    b = dict(batch)
    b["img"] = batch["img"].detach().clone().requires_grad_(want_img_grad)
    m.zero_grad(set_to_none=True)
    _, loss = m(b)
    sum(loss.values()).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    bufs = {n: v.detach().clone() for n, v in m.named_buffers()}
    return [v.detach().clone() for v in loss.values()], grads, bufs, (b["img"].grad.clone() if want_img_grad else b["img"].grad)


def _same(a, b, tag):
    assert a.keys() == b.keys() and len(a) > 0, tag
    for n in a:
        assert torch.equal(a[n], b[n]), (tag, n)


@pytest.mark.parametrize("env", [{"MONOCON_HIP_GRAD_POOL": "0"}, {"MONOCON_HIP_GRAD_POOL": "1"}, {"MONOCON_HIP_DUAL_STREAM": "0"}],
                         ids=["private-buffers", "grad-pool", "one-stream"])
def test_asking_for_the_image_gradient_changes_nothing_else(golden_sd, env, monkeypatch):
    """fresh f16x2 models on one batch: the ten losses, every parameter gradient and every running buffer of a step with
    img.requires_grad equal those of a step without it bit for bit; two requesting steps give the same img.grad; a third
    step that stops asking gives the first step's parameter gradients again (no stale pointer, no leftover state).  The
    later steps start from the fresh model's running buffers again (_restore)."""
    _clean_env(monkeypatch, env)
    batch = to_cuda(synth.make_batch(77, 2, 64, 128))
    plain = build(golden_sd, "f16x2")
    L0, G0, B0, none = _step(plain, batch, False)
    assert none is None and len(G0) == 236
    del plain
    asking = build(golden_sd, "f16x2")
    fresh = _buffers(asking)
    L1, G1, B1, gi1 = _step(asking, batch, True)
    assert gi1 is not None and bool(torch.isfinite(gi1).all()) and float(gi1.abs().max()) > 0
    assert all(torch.equal(a, b) for a, b in zip(L0, L1)) and len(L1) == 10
    _same(G0, G1, "parameter gradients")
    _same(B0, B1, "running buffers")
    _restore(asking, fresh)
    L2, G2, _, gi2 = _step(asking, batch, True)
    assert torch.equal(gi1, gi2)
    _same(G1, G2, "parameter gradients of the second asking step")
    _restore(asking, fresh)
    L3, G3, B3, none = _step(asking, batch, False)
    assert none is None
    _same(G1, G3, "parameter gradients of the step that stopped asking")
    _same(B1, B3, "running buffers of the step that stopped asking")
    assert all(torch.equal(a, b) for a, b in zip(L1, L3))


# ------------------------------------------------------------------------------------------------ 4: autograd semantics
SEM_SHAPE = (2, 64, 64)
SEM_SEED = 419


@pytest.fixture(scope="module")
def sem(cond_sd):
    """the model and batch of the semantics tests, its fresh running buffers (every step below starts from them: _restore)
    and d sum(losses) / d img of that batch"""
    B, H, W = SEM_SHAPE
    batch = to_cuda(synth.make_conditioned_batch(SEM_SEED, B, H, W))
    m = build(cond_sd, "f16x2")
    fresh = _buffers(m)
    b = dict(batch)
    b["img"] = batch["img"].detach().clone().requires_grad_()
    _, loss = m(b)
    sum(loss.values()).backward()
    torch.cuda.synchronize()
    return m, batch, b["img"].grad.detach().clone(), fresh


def _oracle_img_grad(sd, batch, objective, dtype, img=None):
    from oracle import monocon_oracle as O
    live = {k: (v.to(dtype).clone() if v.dtype == torch.float32 else v.clone()) for k, v in sd.items()}
    b = dict(batch)
    b["img"] = (batch["img"] if img is None else img).to(dtype).clone().requires_grad_(True)
    preds, _, L, _ = O.train_forward(live, b)
    objective(preds, L).backward()
    return b["img"].grad.double()


def test_weighted_objective_with_a_map_term(cond_sd, sem):
    """(2 loss_depth + pred_dict['wh_pred'].sum()).backward() with the image asking: against autograd through the oracle in
    fp64 on the same batch and objective, relative L2 <= 1e-3.

    The fixture is case-0-like, by cond_train's own acceptance applied to the oracle alone on this batch and objective: the
    2x64x64 conditioned batch of seed 419 is the first seed after case 0's 417 whose fp64 image gradient moves < 1e-4 under
    3e-7 relative noise on the image (1.1e-5) and whose fp32 run sits < 2e-4 from its fp64 run (2.3e-5 with 8 threads, 2.4e-5
    with one; seed 417 itself: 2.1e-4, seed 418: 3.4e-3).  The test re-checks that selection and asserts it, so a drift of the
    fixture is noticed instead of silently loosening the gate.  Measured on an MI355X: 2.1e-5."""
    m, batch, _, fresh = sem
    _restore(m, fresh)
    cpu = synth.make_conditioned_batch(SEM_SEED, *SEM_SHAPE)
    obj = lambda p, L: 2 * L["loss_depth"] + p["wh_pred"].sum()          # noqa: E731
    g64 = _oracle_img_grad(cond_sd, cpu, obj, torch.float64)
    noise = torch.from_numpy(synth.uniform(SEM_SEED, "cond.noise", tuple(cpu["img"].shape), -1.0, 1.0))
    margin = rel_l2(_oracle_img_grad(cond_sd, cpu, obj, torch.float64, cpu["img"].double() * (1.0 + 3e-7 * noise)), g64)
    e32 = rel_l2(_oracle_img_grad(cond_sd, cpu, obj, torch.float32), g64)
    assert margin < 1e-4 and e32 < 2e-4, "the fixture is no longer case-0-like: perturbed %.3g, fp32 %.3g" % (margin, e32)
    b = dict(batch)
    b["img"] = batch["img"].detach().clone().requires_grad_()
    pred, loss = m(b)
    (2 * loss["loss_depth"] + pred["wh_pred"].sum()).backward()
    torch.cuda.synchronize()
    e = rel_l2(b["img"].grad, g64)
    _say("weighted objective: oracle perturbed-fp64 %.3g, fp32-vs-fp64 %.3g; HIP vs fp64 %.3g (gate 1e-3)" % (margin, e32, e))
    assert e <= 1e-3, e


def test_non_leaf_image(sem):
    """img = 2 * x for a leaf x: autograd chains the image gradient into x, x.grad == 2 * (d / d img) exactly"""
    m, batch, gimg, fresh = sem
    _restore(m, fresh)
    x = (batch["img"].detach() * 0.5).requires_grad_()
    b = dict(batch)
    b["img"] = 2 * x
    assert torch.equal(b["img"].detach(), batch["img"])
    _, loss = m(b)
    sum(loss.values()).backward()
    torch.cuda.synchronize()
    assert torch.equal(x.grad, 2 * gimg)


def test_image_gradient_accumulates(sem):
    """two backwards of two forwards on one leaf image accumulate into img.grad"""
    m, batch, gimg, fresh = sem
    b = dict(batch)
    b["img"] = batch["img"].detach().clone().requires_grad_()
    for _ in range(2):
        _restore(m, fresh)
        _, loss = m(b)
        sum(loss.values()).backward()
    torch.cuda.synchronize()
    assert torch.equal(b["img"].grad, gimg + gimg)


def test_heads_only_plan_refuses_the_image_gradient(cond_sd):
    """mc_backward_image_grad on a handle that holds a heads-only plan fails with a message (that plan has grad_feat)"""
    from model import MonoConDenseHeads
    B, H, W = 2, 64, 64
    batch = synth.make_conditioned_batch(812, B, H, W)
    heads = MonoConDenseHeads(test_config=None)
    heads.load_state_dict({k[5:]: v for k, v in cond_sd.items() if k.startswith("head.")}, strict=True)
    heads = heads.cuda().train()
    feat = torch.from_numpy(synth.normalish(5, "feat", (B, 64, H // 4, W // 4)).astype(np.float32)).abs().cuda()
    data = {"label": {k: v.cuda() for k, v in batch["label"].items()}, "img_metas": batch["img_metas"]}
    heads.forward_train(feat, data)
    eng = heads._rt.engine
    gl = torch.ones(10, device="cuda")
    out = torch.zeros((B, 3, H, W), device="cuda")
    rc = eng.lib.mc_backward_image_grad(eng.h, C.c_void_p(gl.data_ptr()), None, C.c_void_p(out.data_ptr()), _stream())
    torch.cuda.synchronize()
    assert rc != 0
    msg = eng.lib.mc_last_error(eng.h).decode()
    assert "heads-only plan" in msg and "mc_backward_image_grad" in msg, msg
    assert float(out.abs().max()) == 0.0


def test_null_grad_img_is_mc_backward(sem):
    """mc_backward_image_grad(grad_preds = NULL, grad_img = NULL) writes bit-identical parameter gradients to mc_backward"""
    m, batch, _, fresh = sem
    eng, tb = m._rt.engine, m._train_binding
    gl = torch.ones(10, device="cuda")
    flat = []
    for which in ("mc_backward", "mc_backward_image_grad"):
        m.zero_grad(set_to_none=True)
        _restore(m, fresh)
        m(dict(batch))
        if which == "mc_backward":
            rc = eng.lib.mc_backward(eng.h, C.c_void_p(gl.data_ptr()), _stream())
        else:
            rc = eng.lib.mc_backward_image_grad(eng.h, C.c_void_p(gl.data_ptr()), None, None, _stream())
        assert rc == 0, eng.lib.mc_last_error(eng.h)
        torch.cuda.synchronize()
        flat.append({n: g.detach().clone() for n, g in tb.grads.items()})
    _same(flat[0], flat[1], "parameter gradients")
    assert len(flat[0]) == 236 and any(float(g.abs().max()) > 0 for g in flat[0].values())


# ------------------------------------------------------------------------------------------------ 5: op level
@pytest.fixture(scope="module")
def eng():
    from hipmonocon.engine import Engine
    return Engine()


def _rnd(seed, name, shape, std=1.0):
    return torch.from_numpy(synth.normalish(seed, name, shape).astype(np.float32)) * std


def _op_dgrad(eng, dy_nchw, w, y_nchw=None, coef=None):
    """mc_op_stem_dgrad (or its fused door) on CPU tensors: NCHW (B,16,H,W) in, NCHW (B,3,H,W) out"""
    B, _, H, W = dy_nchw.shape
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().cuda()          # noqa: E731
    dy, wd = nhwc(dy_nchw), w.contiguous().cuda()
    out = torch.full((B, 3, H, W), float("nan"), device="cuda")
    if y_nchw is None:
        rc = eng.lib.mc_op_stem_dgrad(eng.h, C.c_void_p(dy.data_ptr()), C.c_void_p(wd.data_ptr()), B, H, W, C.c_void_p(out.data_ptr()),
                                      _stream())
    else:
        yd, cf = nhwc(y_nchw), coef.contiguous().cuda()
        rc = eng.lib.mc_op_stem_dgrad_fused(eng.h, C.c_void_p(dy.data_ptr()), C.c_void_p(yd.data_ptr()), C.c_void_p(cf.data_ptr()),
                                            C.c_void_p(wd.data_ptr()), B, H, W, C.c_void_p(out.data_ptr()), _stream())
    assert rc == 0, eng.lib.mc_last_error(eng.h)
    torch.cuda.synchronize()
    return out.cpu()


def _check_op(tag, got, dY64, w, extra=None):
    shape = (dY64.shape[0], 3) + tuple(dY64.shape[2:])
    ref = torch.nn.grad.conv2d_input(shape, w.double(), dY64, padding=3)
    mag = torch.nn.grad.conv2d_input(shape, w.double().abs(), dY64.abs(), padding=3)
    f32 = torch.nn.grad.conv2d_input(shape, w.float(), dY64.float(), padding=3)
    assert bool(torch.isfinite(got).all()), tag + ": an output element was not written"
    e, yard, of_gate = _conv_gate(got, ref, mag, f32, extra)
    _say("%s: HIP %.3g / float32 %.3g, %.3g of the gate" % (tag, e, yard, of_gate))
    assert of_gate <= 1.0, (tag, e, yard, of_gate)


OP_SHAPES = [(1, 7, 9), (2, 13, 37), (2, 70, 203), (3, 32, 96)]


@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_op_stem_dgrad(eng, shape):
    """smaller than a tile and narrower than two halos; odd sizes; several ragged tiles in both directions; a plan-sized map"""
    B, H, W = shape
    w = _rnd(11, "stem.w", (16, 3, 7, 7), 0.1)
    dy = _rnd(12 + W, "stem.dy", (B, 16, H, W))
    _check_op("stored %dx%dx%d" % shape, _op_dgrad(eng, dy, w), dy.double(), w)


@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_op_stem_dgrad_corner_impulse(eng, shape):
    """dY = a single 1 in the last corner: the output is the weight's flipped footprint clipped by the map (the padding made
    visible), exactly -- one product per output element"""
    B, H, W = shape
    w = _rnd(11, "stem.w", (16, 3, 7, 7), 0.1)
    dy = torch.zeros((B, 16, H, W))
    dy[B - 1, 5, H - 1, W - 1] = 1.0
    got = _op_dgrad(eng, dy, w)
    ref = torch.nn.grad.conv2d_input((B, 3, H, W), w.double(), dy.double(), padding=3)
    assert torch.equal(got.double(), ref)
    assert int((got != 0).sum()) == 3 * min(4, H) * min(4, W)


@pytest.mark.parametrize("shape", [(2, 13, 37), (2, 70, 203)], ids=lambda s: "%dx%dx%d" % s)
def test_op_stem_dgrad_fused(eng, shape):
    """the fused door: dY = P d + Q y + R formed while the tile is staged, random P, Q, R per channel, about half of d zero"""
    B, H, W = shape
    w = _rnd(11, "stem.w", (16, 3, 7, 7), 0.1)
    d = _rnd(31 + W, "stem.d", (B, 16, H, W))
    d = d * (_rnd(32 + W, "stem.mask", (B, 16, H, W)) > 0)
    y = _rnd(33 + W, "stem.y", (B, 16, H, W), 2.0)
    coef = torch.zeros((16, 4))
    coef[:, :3] = _rnd(34, "stem.coef", (16, 3))
    assert 0.4 < float((d == 0).float().mean()) < 0.6
    v = lambda k: coef[:, k].double()[None, :, None, None]          # noqa: E731
    dY = v(0) * d.double() + v(1) * y.double() + v(2)
    terms = v(0).abs() * d.double().abs() + v(1).abs() * y.double().abs() + v(2).abs()
    extra = torch.nn.grad.conv2d_input((B, 3, H, W), w.double().abs(), 8 * U * terms, padding=3)
    _check_op("fused %dx%dx%d" % shape, _op_dgrad(eng, d, w, y, coef), dY, w, extra)
