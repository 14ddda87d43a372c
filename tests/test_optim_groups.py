"""The fused AdamW beyond the reference's single recipe -- parameter groups, per-parameter step counts, amsgrad, maximize, any
clip norm -- and the stand-alone fused clip_grad_norm_, against ``torch.optim.AdamW`` + ``torch.nn.utils.clip_grad_norm_`` on CPU
float32 copies of the same tensors.  Tolerances are the project's own for this arithmetic (test_hip_train_pieces.py,
test_fused_clip_matches_torch_clip): rel_err < 2e-6 per tensor after three steps, norms within rel 1e-5.

The tensor set reaches every path of the kernels' chunk walk: a 16-byte-aligned body with and without a scalar tail, a single
element, a tensor that crosses the 65536-element chunk boundary, a gradient that is 4- but not 16-byte aligned (a slice at
element offset 1 of a larger buffer), and 2100 five-element tensors, which make more chunks (2107) than the launch has
workgroups (2048): workgroups 0..58 walk a second chunk, and it belongs to another group than their first."""
import ctypes as C
import math

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

BIG = [(64, 32, 3, 3), (131,), (1,), (10, 64), (70000,), (37,)]
MISALIGNED = 5                      # index of the tensor whose gradient sits at element offset 1 of its buffer
N_SMALL = 2100
N_ALL = len(BIG) + N_SMALL
TOL, NORM_TOL = 2e-6, 1e-5
# Clipped at p = 1 and p = 3, the CPU oracle's own float32 norm is the largest error in the comparison: the clip coefficient
# inherits it, exp_avg and every clipped gradient carry it once, exp_avg_sq twice.  torch's CPU float32 result against the same
# torch code in float64 on these very inputs (three clipped steps, the groups of test_clip_norm_types) is off by
#   p = 1: norm 2.42e-6, exp_avg 1.16e-6, exp_avg_sq 2.45e-6, parameters 3.4e-7
#   p = 3: norm 1.97e-6, exp_avg 1.64e-6, exp_avg_sq 3.19e-6, parameters 3.4e-7
# (p = 2: 1.4e-7 / 1.1e-7 / 1.9e-7 / 3.4e-7; p = inf: 0 / 1.4e-7 / 2.8e-7 / 3.4e-7: inside TOL), so those two norm types
# allow twice the oracle's own error on the moments and on a clipped gradient; parameters stay at TOL for every norm type.
ORACLE_NORM_ERR = {1.0: 2.42e-6, 3.0: 1.97e-6}
ORACLE_MOMENT_ERR = {1.0: 2.45e-6, 3.0: 3.19e-6}
HYPER = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)


@pytest.fixture(scope="module")
def data():
    """(initial values, gradients) on the CPU; never modified -- every test clones what it needs"""
    gen = torch.Generator().manual_seed(0)
    shapes = BIG + [(5,)] * N_SMALL
    base = [torch.randn(s, generator=gen) for s in shapes]
    grads = [torch.randn(s, generator=gen) * 3 for s in shapes]
    return base, grads


def two_groups():
    big = list(range(len(BIG)))
    small = list(range(len(BIG), N_ALL))
    return big[0::2] + small[0::2], big[1::2] + small[1::2]


def device_grad(g, misaligned):
    if not misaligned:
        return g.cuda()
    buf = torch.zeros(g.numel() + 8, device="cuda")
    view = buf[1:1 + g.numel()].view(g.shape)
    view.copy_(g)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


class Pair:
    """the fused optimizer on the device beside torch.optim.AdamW on the CPU, over the same groups"""

    def __init__(self, data, groups, max_norm=None, norm_type=2.0, **defaults):
        from solver import AdamW
        self.base, self.grads = data
        self.max_norm, self.norm_type = max_norm, norm_type
        self.pa, self.pb = {}, {}
        kw = dict(HYPER)
        kw.update(defaults)
        self.oa = AdamW(self._groups(groups, self.pa, True), max_grad_norm=max_norm, norm_type=norm_type, **kw)
        self.ob = torch.optim.AdamW(self._groups(groups, self.pb, False), **kw)

    def _groups(self, groups, store, dev):
        out = []
        for ids, over in groups:
            for i in ids:
                b = self.base[i].clone()
                store[i] = torch.nn.Parameter(b.cuda() if dev else b)
            out.append(dict(params=[store[i] for i in ids], **over))
        return out

    def add_group(self, ids, **over):
        self.oa.add_param_group(self._groups([(ids, over)], self.pa, True)[0])
        self.ob.add_param_group(self._groups([(ids, over)], self.pb, False)[0])

    def set_grads(self, scale, skip=()):
        for i in self.pa:
            if i in skip:
                self.pa[i].grad = self.pb[i].grad = None
                continue
            g = self.grads[i] * scale
            self.pb[i].grad = g.clone()
            self.pa[i].grad = device_grad(g, i == MISALIGNED)

    def step(self):
        ref_norm = None
        if self.max_norm is not None:
            ref_norm = torch.nn.utils.clip_grad_norm_(list(self.pb.values()), self.max_norm, norm_type=self.norm_type)
        self.oa.step()
        self.ob.step()
        return ref_norm

    def check(self, moment_tol=TOL):
        for i in self.pa:
            e = rel_err(self.pa[i], self.pb[i])
            assert e < TOL, ("param", i, e)
            sa, sb = self.oa.state.get(self.pa[i], {}), self.ob.state.get(self.pb[i], {})
            assert set(sa) == set(sb), (i, set(sa), set(sb))
            if not sb:
                continue
            assert float(sa["step"]) == float(sb["step"]), (i, float(sa["step"]), float(sb["step"]))
            for k in sb:
                if k != "step":
                    e = rel_err(sa[k], sb[k])
                    assert e < moment_tol, (k, i, e)


def test_three_groups_with_a_cyclic_schedule(data):
    """(1) three groups, each with its own lr / betas / eps / weight_decay, a one-cycle schedule over all of them; the table is
    bound once although lr and beta1 move every step"""
    from solver import CyclicScheduler
    g0, g1 = two_groups()
    g0.remove(4)
    pr = Pair(data, [(g0, {}),(g1, dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.0)),
                     ([4], dict(lr=2e-4, betas=(0.95, 0.999), eps=1e-7, weight_decay=0.1))], max_norm=5.0)
    sch = [CyclicScheduler(o, total_steps=10, target_lr_ratio=(10, 1e-4), target_momentum_ratio=(0.85 / 0.95, 1.0), period_up=0.4)
           for o in (pr.oa, pr.ob)]
    pr.set_grads(1.0)
    bufs = {i: p.grad for i, p in pr.pa.items()}
    sig = None
    for it in range(3):
        for i, p in pr.pa.items():              # the same gradient buffers every step, as a train loop's
            bufs[i].copy_(data[1][i] * (it + 1))
            p.grad = bufs[i]
            pr.pb[i].grad = data[1][i] * (it + 1)
        assert [g["lr"] for g in pr.oa.param_groups] == [g["lr"] for g in pr.ob.param_groups]
        assert len({g["lr"] for g in pr.oa.param_groups}) == 3
        ref_norm = pr.step()
        assert float(pr.oa.last_grad_norm) == pytest.approx(float(ref_norm), rel=NORM_TOL)
        if sig is not None:
            assert pr.oa._bound_sig is sig, "re-bound although no pointer and no class index changed"
        sig = pr.oa._bound_sig
        for s in sch:
            s.step()
    pr.check()


def _old_entry_run(data, ids, max_norm, steps=3):
    """the reference recipe through the original C entry points (mc_optim_bind + mc_clip_adamw_step), no Python optimizer"""
    from hipmonocon import lib as L
    from hipmonocon.engine import Engine
    eng = Engine(0)
    p = [data[0][i].clone().cuda() for i in ids]
    g = [device_grad(data[1][i], i == MISALIGNED) for i in ids]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    n = len(ids)
    arr = [(C.c_void_p * n)(*[t.data_ptr() for t in ts]) for ts in (p, g, m, v)]
    numel = (C.c_int64 * n)(*[t.numel() for t in p])
    L.check(eng.h, eng.lib.mc_optim_bind(eng.h, n, arr[0], arr[1], arr[2], arr[3], numel), "mc_optim_bind")
    norm = torch.zeros(1, device="cuda")
    for it in range(steps):
        for t, i in zip(g, ids):
            t.copy_(data[1][i] * (it + 1))
        rc = eng.lib.mc_clip_adamw_step(eng.h, HYPER["lr"], HYPER["betas"][0], HYPER["betas"][1], HYPER["eps"],
                                        HYPER["weight_decay"], float(max_norm or 0.0), it + 1, C.c_void_p(norm.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
        L.check(eng.h, rc, "mc_clip_adamw_step")
    torch.cuda.synchronize()
    return p, m, v, norm


@pytest.mark.parametrize("max_norm", (None, 5.0))
def test_split_into_equal_groups_is_bit_identical_to_the_old_entry_point(data, max_norm):
    """(2) one list split in order into two groups with equal hyper-parameters folds into one class: the launch, and every bit of
    the parameters, the moments and the norm, are those of the single group through mc_optim_bind + mc_clip_adamw_step"""
    ids = list(range(N_ALL))
    half = N_ALL // 2
    p, m, v, norm = _old_entry_run(data, ids, max_norm)
    pr = Pair(data, [(ids[:half], {}), (ids[half:], {})], max_norm=max_norm)
    for it in range(3):
        pr.set_grads(it + 1)
        pr.step()
    for k, i in enumerate(ids):
        st = pr.oa.state[pr.pa[i]]
        assert torch.equal(pr.pa[i].detach(), p[k]), i
        assert torch.equal(st["exp_avg"], m[k]) and torch.equal(st["exp_avg_sq"], v[k]), i
    assert torch.equal(pr.oa.last_grad_norm, norm)
    pr.check()


def test_a_gradient_that_first_appears_at_step_two(data):
    """(3) torch keeps the step per parameter: a late parameter has its own bias correction"""
    g0, g1 = two_groups()
    pr = Pair(data, [(g0, {}), (g1, dict(lr=2e-3))], max_norm=5.0)
    late = (3, 4, 11)
    for it in range(3):
        pr.set_grads(it + 1, skip=late if it == 0 else ())
        ref_norm = pr.step()
        assert float(pr.oa.last_grad_norm) == pytest.approx(float(ref_norm), rel=NORM_TOL)
    for i in pr.pa:
        assert float(pr.oa.state[pr.pa[i]]["step"]) == (2.0 if i in late else 3.0)
    pr.check()


def test_add_param_group_after_a_step(data):
    """(4) a group added mid-run starts at step 1 beside parameters at step 2"""
    g0, g1 = two_groups()
    pr = Pair(data, [(g0, {})])
    pr.set_grads(1.0)
    pr.step()
    pr.add_group(g1, lr=5e-3, weight_decay=0.0)
    for it in (1, 2):
        pr.set_grads(it + 1)
        pr.step()
    assert float(pr.oa.state[pr.pa[g0[0]]]["step"]) == 3.0 and float(pr.oa.state[pr.pa[g1[0]]]["step"]) == 2.0
    pr.check()


@pytest.fixture(scope="module")
def ref_norms(data):
    """torch's norms of the step-1 gradients of the whole set, per norm type"""
    ps = []
    for g in data[1]:
        p = torch.nn.Parameter(torch.zeros_like(g))
        p.grad = g.clone()
        ps.append(p)
    return {p: float(torch.nn.utils.clip_grad_norm_(ps, 1e30, norm_type=p)) for p in (1.0, 2.0, 3.0, math.inf)}


@pytest.mark.parametrize("norm_type", (1.0, 2.0, 3.0, math.inf))
@pytest.mark.parametrize("case", ("above", "below", "zero"))
def test_clip_norm_types(data, ref_norms, norm_type, case):
    """(5) the step's clip for p in {1, 2, 3, inf}: clipped (the norm is twice max_norm), not clipped (half of it), and all-zero
    gradients, whose coefficient max_norm / (0 + 1e-6) clamps to 1"""
    g0, g1 = two_groups()
    max_norm = ref_norms[norm_type] * {"above": 0.5, "below": 2.0, "zero": 1.0}[case]
    pr = Pair(data, [(g0, {}), (g1, dict(lr=2e-3))], max_norm=max_norm, norm_type=norm_type)
    for it in range(3):
        pr.set_grads(0.0 if case == "zero" else 1.0 + 0.25 * it)
        ref_norm = pr.step()
        if case == "zero":
            assert float(pr.oa.last_grad_norm) == 0.0 == float(ref_norm)
        else:
            assert float(pr.oa.last_grad_norm) == pytest.approx(float(ref_norm), rel=NORM_TOL)
            assert (float(ref_norm) > max_norm) == (case == "above")      # 2x .. 3x max_norm, or 0.5x .. 0.75x
    pr.check(moment_tol=2 * ORACLE_MOMENT_ERR[norm_type] if case == "above" and norm_type in ORACLE_MOMENT_ERR else TOL)


def test_amsgrad_beside_a_plain_group(data):
    """(6) gradients shrink at step 2 and stay small, so exp_avg_sq falls below its running maximum and vmax != v from then on.
    The L2 norm of the set is about 950 x scale: max_norm 2000 clips the first step only (a clip at every step would undo the
    shrinking).  With beta2 = 0.99 and g the first step's clipped gradient: v1 = 0.01 g^2 = vmax, v2 = 0.00994 g^2,
    v3 = 0.00998 g^2"""
    g0, g1 = two_groups()
    pr = Pair(data, [(g0, dict(amsgrad=True)), (g1, {})], max_norm=2000.0)
    for scale, clipped in ((3.0, True), (0.1, False), (0.2, False)):
        pr.set_grads(scale)
        assert (float(pr.step()) > 2000.0) == clipped
    sa = pr.oa.state[pr.pa[4]]
    assert "max_exp_avg_sq" in sa and "max_exp_avg_sq" not in pr.oa.state[pr.pa[g1[0]]]
    assert bool((sa["max_exp_avg_sq"] > sa["exp_avg_sq"]).any())
    sb = pr.ob.state[pr.pb[4]]
    assert bool((sb["max_exp_avg_sq"] > sb["exp_avg_sq"]).all())
    pr.check()


def test_maximize_group(data):
    """(7) maximize flips the gradient's sign after the clip coefficient"""
    g0, g1 = two_groups()
    pr = Pair(data, [(g0, dict(maximize=True)), (g1, {})], max_norm=5.0)
    for it in range(3):
        pr.set_grads(it + 1)
        pr.step()
    pr.check()
    pr1 = Pair(data, [(g0 + g1, {})], max_norm=5.0, maximize=True)      # one class with a flag: the class kernel, not the default
    for it in range(3):
        pr1.set_grads(it + 1)
        pr1.step()
    pr1.check()


def test_a_group_held_still_with_lr_zero(data):
    """(8) lr = 0 and weight_decay = 0: the parameters keep every bit, the moments advance"""
    g0, g1 = two_groups()
    pr = Pair(data, [(g0, {}), (g1, dict(lr=0.0, weight_decay=0.0))], max_norm=5.0)
    for it in range(3):
        pr.set_grads(it + 1)
        pr.step()
    for i in g1:
        assert torch.equal(pr.pa[i].detach().cpu(), data[0][i]), i
        assert float(pr.oa.state[pr.pa[i]]["exp_avg"].abs().max()) > 0
    assert not torch.equal(pr.pa[0].detach().cpu(), data[0][0])
    pr.check()


@pytest.mark.parametrize("norm_type", (1.0, 2.0, 3.0, math.inf))
def test_standalone_clip_grad_norm(data, ref_norms, norm_type):
    """(9) solver.clip_grad_norm_ against torch's, clipped and not"""
    from solver import clip_grad_norm_
    for factor in (0.5, 2.0):
        max_norm = ref_norms[norm_type] * factor
        pa = [torch.nn.Parameter(torch.zeros_like(g).cuda()) for g in data[1]]
        pb = [torch.nn.Parameter(torch.zeros_like(g)) for g in data[1]]
        for i, (p, q, g) in enumerate(zip(pa, pb, data[1])):
            p.grad, q.grad = device_grad(g, i == MISALIGNED), g.clone()
        ref = torch.nn.utils.clip_grad_norm_(pb, max_norm, norm_type=norm_type)
        got = clip_grad_norm_(pa, max_norm, norm_type=norm_type)
        assert got.is_cuda and float(got) == pytest.approx(float(ref), rel=NORM_TOL)
        for i, (p, q) in enumerate(zip(pa, pb)):
            if factor > 1.0:
                assert torch.equal(p.grad.cpu(), data[1][i]), i       # coefficient 1: untouched
            assert rel_err(p.grad, q.grad) < (2 * ORACLE_NORM_ERR[norm_type] if factor < 1.0 and norm_type in ORACLE_NORM_ERR else TOL), i


def test_standalone_clip_then_plain_step_is_the_fused_clipped_step(data):
    """(9) clip_grad_norm_ followed by an unclipped fused step == the fused clipped step, bit for bit at p = 2"""
    from solver import clip_grad_norm_
    ids = list(range(N_ALL))
    a = Pair(data, [(ids, {})], max_norm=None)
    b = Pair(data, [(ids, {})], max_norm=5.0)
    from hipmonocon.engine import Engine
    eng = Engine(0)                         # one handle for both: the clip's gradient table sits beside the optimizer's
    a.oa.set_engine(eng)
    for it in range(2):
        a.set_grads(it + 1)
        b.set_grads(it + 1)
        n = clip_grad_norm_(list(a.pa.values()), 5.0, engine=eng)
        a.oa.step()
        b.oa.step()
        assert torch.equal(n.reshape(1), b.oa.last_grad_norm)
    for i in ids:
        assert torch.equal(a.pa[i].detach(), b.pa[i].detach()), i
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a.oa.state[a.pa[i]][k], b.oa.state[b.pa[i]][k]), (k, i)


def test_checkpoints_move_both_ways(data):
    """(10) state_dict() of the fused optimizer (two groups, one amsgrad) loads into torch.optim.AdamW and back; a
    torch.optim.AdamW state dict with two groups loads into the fused optimizer; the next step matches either way"""
    g0, g1 = two_groups()
    groups = [(g0, dict(amsgrad=True)), (g1, dict(lr=2e-3))]
    src = Pair(data, groups, max_norm=5.0)
    for it in range(2):
        src.set_grads(it + 1)
        src.step()
    sd_fused, sd_torch = src.oa.state_dict(), src.ob.state_dict()
    assert set(sd_fused) == set(sd_torch) and len(sd_fused["param_groups"]) == 2
    for ga, gb in zip(sd_fused["param_groups"], sd_torch["param_groups"]):
        assert set(ga) == set(gb) and ga["params"] == gb["params"]
    assert all(set(sd_fused["state"][k]) == set(sd_torch["state"][k]) for k in sd_torch["state"])
    # fused -> torch, and fused -> torch -> fused
    dst = Pair(data, groups, max_norm=5.0)
    for i in src.pa:
        dst.pa[i].data.copy_(src.pa[i].data)
        dst.pb[i].data.copy_(src.pa[i].data.cpu())
    dst.ob.load_state_dict(sd_fused)
    dst.oa.load_state_dict(dst.ob.state_dict())
    dst.set_grads(3.0)
    dst.step()
    dst.check()
    assert float(dst.oa.state[dst.pa[0]]["step"]) == 3.0
    # torch -> fused
    dst = Pair(data, groups, max_norm=5.0)
    for i in src.pb:
        dst.pa[i].data.copy_(src.pb[i].data)
        dst.pb[i].data.copy_(src.pb[i].data)
    dst.oa.load_state_dict(sd_torch)
    dst.ob.load_state_dict(sd_torch)
    assert dst.oa.state[dst.pa[0]]["max_exp_avg_sq"].is_cuda
    dst.set_grads(3.0)
    dst.step()
    dst.check()


def _engine_cfg(tmp_path, **optim):
    from utils.engine_utils import get_default_cfg
    cfg = get_default_cfg()
    cfg.set_new_allowed(True)
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.SEED = 3
    cfg.DATA.ROOT = 'synthetic'
    cfg.DATA.SYNTHETIC_LENGTH = 4
    cfg.DATA.SYNTHETIC_HW = [96, 224]
    cfg.DATA.BATCH_SIZE = 2
    cfg.DATA.NUM_WORKERS = 0
    cfg.MODEL.BACKBONE.IMAGENET_PRETRAINED = False
    cfg.SOLVER.OPTIM.NUM_EPOCHS = 1
    cfg.PERIOD.EVAL_PERIOD = 0
    cfg.PERIOD.LOG_PERIOD = 1
    return cfg


def _two_engine_steps(cfg, tmp_path, tag, patch=None):
    import os
    from engine.monocon_engine import MonoconEngine
    from utils.engine_utils import set_random_seed
    set_random_seed(3)
    cfg.OUTPUT_DIR = os.path.join(str(tmp_path), tag)
    os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
    eng = MonoconEngine(cfg)
    if patch is not None:
        patch(eng)
    before = {k: v.detach().clone() for k, v in eng.model.named_parameters()}
    eng.train_one_epoch()
    torch.cuda.synchronize()
    assert len(eng.entire_losses) == 2
    return eng, before


def test_engine_freezes_the_backbone_through_the_optimizer(tmp_path):
    """(11) BACKBONE_LR_MULT 0.0 + NO_DECAY_NORM_BIAS + NORM_TYPE inf: two steps leave every backbone.* parameter bit-unchanged,
    neck and head move, group 0 carries the scheduler's base learning rate"""
    cfg = _engine_cfg(tmp_path)
    cfg.SOLVER.OPTIM.BACKBONE_LR_MULT = 0.0
    cfg.SOLVER.OPTIM.NO_DECAY_NORM_BIAS = True
    cfg.SOLVER.CLIP_GRAD.NORM_TYPE = float("inf")
    eng, before = _two_engine_steps(cfg, tmp_path, "frozen")
    opt = eng.optimizer
    assert len(opt.param_groups) == 4 and opt.norm_type == math.inf
    assert [g["weight_decay"] for g in opt.param_groups] == [cfg.SOLVER.OPTIM.WEIGHT_DECAY, cfg.SOLVER.OPTIM.WEIGHT_DECAY, 0.0, 0.0]
    assert eng.scheduler.base_lrs == [cfg.SOLVER.OPTIM.LR, 0.0, cfg.SOLVER.OPTIM.LR, 0.0]
    assert opt.param_groups[0]["lr"] == eng.scheduler.get_last_lr()[0] == eng.current_lr > 0
    assert opt.param_groups[1]["lr"] == 0.0 and opt.param_groups[3]["lr"] == 0.0
    moved = 0
    for k, v in eng.model.named_parameters():
        if k.startswith("backbone."):
            assert torch.equal(v.detach(), before[k]), k
            if v.grad is not None and bool((v.grad != 0).any()):   # held still by lr = 0, not skipped: its moments advanced
                assert float(opt.state[v]["exp_avg"].abs().max()) > 0, k
        elif v.grad is not None and bool((v.grad != 0).any()):
            assert not torch.equal(v.detach(), before[k]), k
            moved += 1
    assert moved > 50 and bool(torch.isfinite(opt.last_grad_norm).all())


def test_engine_defaults_are_the_single_group_of_before(tmp_path):
    """(11) all three keys at their defaults: one parameter group, and two steps are bit-identical to an engine whose optimizer
    is constructed the way build_solver constructed it before the keys existed"""
    from solver import AdamW, CyclicScheduler

    def as_before(eng):
        cfg = eng.cfg
        eng.optimizer = AdamW(eng.model.parameters(), lr=cfg.SOLVER.OPTIM.LR, weight_decay=cfg.SOLVER.OPTIM.WEIGHT_DECAY,
                              betas=(0.95, 0.99), max_grad_norm=float(cfg.SOLVER.CLIP_GRAD.MAX_NORM))
        eng.scheduler = CyclicScheduler(eng.optimizer, total_steps=len(eng.train_loader) * cfg.SOLVER.OPTIM.NUM_EPOCHS,
                                        target_lr_ratio=(10, 1E-04), target_momentum_ratio=(0.85 / 0.95, 1.0), period_up=0.4)

    a, _ = _two_engine_steps(_engine_cfg(tmp_path), tmp_path, "a")
    assert len(a.optimizer.param_groups) == 1 and a.optimizer.norm_type == 2.0
    b, before = _two_engine_steps(_engine_cfg(tmp_path), tmp_path, "b", patch=as_before)
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert any(not torch.equal(v.detach(), before[k]) for k, v in b.model.named_parameters())
    assert a.entire_losses == b.entire_losses
    assert torch.equal(a.optimizer.last_grad_norm, b.optimizer.last_grad_norm)


def test_argument_errors_return_without_launching(data):
    """(12) every bad argument fails on the host: the call returns an error and the bound tensors keep every bit"""
    from hipmonocon import lib as L
    from hipmonocon.engine import Engine
    from solver import AdamW, clip_grad_norm_
    eng = Engine(0)
    n = 3
    p = [data[0][i].clone().cuda() for i in range(n)]
    g = [data[1][i].clone().cuda() for i in range(n)]
    m, v, x = ([torch.zeros_like(t) for t in p] for _ in range(3))
    keep = [t.clone() for t in p + g + m + v + x]
    arr = [(C.c_void_p * n)(*[t.data_ptr() for t in ts]) for ts in (p, g, m, v, x)]
    numel = (C.c_int64 * n)(*[t.numel() for t in p])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def bind(cls, vmax=arr[4]):
        return eng.lib.mc_optim_bind_classes(eng.h, n, arr[0], arr[1], arr[2], arr[3], vmax, numel, (C.c_int * n)(*cls))

    def step(classes, norm_type=2.0, ncls=None):
        tab = (L.OptimClass * max(len(classes), 1))(*classes)
        return eng.lib.mc_clip_adamw_step_classes(eng.h, tab, len(classes) if ncls is None else ncls, 5.0, norm_type, None, stream)

    def err():
        return eng.lib.mc_last_error(eng.h).decode()

    cl = (1e-3, 0.9, 0.99, 1e-8, 1e-2, 1, 0, 0)
    assert step([cl]) != 0 and "bind" in err()                          # nothing bound yet
    assert bind([0, 16, 0]) != 0 and "class index 16" in err()         # a class index out of range
    assert bind([0, -1, 0]) != 0 and "class index -1" in err()
    assert bind([0, 1, 0]) == 0
    assert step([cl]) != 0 and "class index 1" in err()                 # the table needs two classes
    assert step([cl] * 17) != 0 and "17" in err() and "16" in err()     # 17 classes
    for bad in (0.0, -1.0, math.nan):
        assert step([cl, cl], norm_type=bad) != 0 and "norm_type" in err()
    assert step([cl, cl[:5] + (0, 0, 0)]) != 0 and "step" in err()      # step < 1
    nul = (C.c_void_p * n)(x[0].data_ptr(), None, x[2].data_ptr())
    assert bind([0, 1, 0], vmax=nul) == 0
    assert step([cl, cl[:6] + (1, 0)]) != 0 and "max_exp_avg_sq" in err()   # an amsgrad class with a null fifth pointer
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(p + g + m + v + x, keep))
    assert step([cl[:6] + (1, 0), cl]) == 0                             # ... the class whose tensors carry it is fine
    torch.cuda.synchronize()
    assert not any(torch.equal(a, b) for a, b in zip(p, keep[:n]))
    # the stand-alone clip
    assert eng.lib.mc_clip_grad_norm(eng.h, 1.0, 2.0, None, stream) != 0 and "mc_clip_bind" in err()
    ga = (C.c_void_p * n)(*[t.data_ptr() for t in g])
    assert eng.lib.mc_clip_bind(eng.h, n, ga, numel) == 0
    for bad in (0.0, -2.0, math.nan):
        assert eng.lib.mc_clip_grad_norm(eng.h, 1.0, bad, None, stream) != 0 and "norm_type" in err()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(g, keep[n:2 * n]))
    # and through Python
    q = [torch.nn.Parameter(t.clone()) for t in p]
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError):
            AdamW(q, norm_type=bad)
        with pytest.raises(ValueError):
            clip_grad_norm_(q, 1.0, norm_type=bad)
    many = [torch.nn.Parameter(torch.ones(4, device="cuda")) for _ in range(17)]
    opt = AdamW([dict(params=[t], lr=1e-3 * (k + 1)) for k, t in enumerate(many)])
    for t in many:
        t.grad = torch.ones_like(t)
    with pytest.raises(L.MonoconHipError, match="more than 16"):
        opt.step()
    assert all(torch.equal(t.detach(), torch.ones_like(t)) for t in many)
    opt.param_groups[16]["lr"] = opt.param_groups[15]["lr"]             # 16 classes fit
    opt.step()
    assert all(float(opt.state[t]["step"]) == 1.0 for t in many)
    assert not torch.equal(many[0].detach(), torch.ones_like(many[0]))
