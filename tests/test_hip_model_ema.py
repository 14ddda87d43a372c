"""ModelEMA on the GPU: the stand-alone multi-tensor average (``mc_ema_bind`` / ``mc_ema_update``) against the fp64 recurrence,
the average fused into the AdamW pass (``mc_optim_bind_ema`` / ``mc_clip_adamw_ema_step_classes``) against the stand-alone one
bit for bit, the argument checks, and the feature through the detector and the engine.

The bound of an averaged element after T updates: one update is ``e' = fl(e + fl(w) * fl(x - e))`` -- two fp32 roundings
(2 * 2^-24 relative to the values at hand) plus the rounding of w to fp32 (2^-24), and the error an earlier update left only
shrinks by (1 - w).  Doubled: ``|e - e_fp64| <= T * 2^-22 * M`` element-wise, M the largest of |e| and |x| seen at that element.
"""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 65536
SIZES = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7)
WEIGHTS = (0.5, 1e-3, 2e-4, 0.1)
EPS = 2.0 ** -22


def misaligned(t):
    """a contiguous copy of ``t`` that starts one float into its storage: 4- but not 16-byte aligned"""
    buf = torch.zeros(t.numel() + 8, device="cuda", dtype=t.dtype)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check_bound(e, e64, M, T, what):
    err = (e.detach().cpu().double() - e64).abs()
    lim = T * EPS * M
    worst = float((err - lim).max())
    print("%s: max |e - e64| = %.3e, largest err / bound = %.3f" % (what, float(err.max()), float((err / lim.clamp_min(1e-300)).max())))
    assert worst <= 0.0, (what, float(err.max()), worst)


# ------------------------------------------------------------------------------------------------ 1. stand-alone kernel
@pytest.fixture(scope="module")
def pairs():
    """(initial averages, one source per update) on the CPU; never modified"""
    gen = torch.Generator().manual_seed(11)
    e0 = [torch.randn(n, generator=gen) for n in SIZES]
    srcs = [[torch.randn(n, generator=gen) * (1 + t) for n in SIZES] for t in range(len(WEIGHTS))]
    return e0, srcs


def bind_pairs(eng, e, s):
    n = len(e)
    numel = (C.c_int64 * n)(*[t.numel() for t in e])
    return eng.lib.mc_ema_bind(eng.h, n, ptr_array(e), ptr_array(s), numel)


def device_pairs(e0, src):
    """the averages and sources on the device: the average of the 65537-element tensor and the source of the 5-element one
    start one float into their storage"""
    e = [misaligned(t) if t.numel() == CHUNK + 1 else t.clone().cuda() for t in e0]
    s = [misaligned(t) if t.numel() == 5 else t.clone().cuda() for t in src]
    return e, s


def test_standalone_kernel_against_fp64(pairs):
    from hipmonocon.engine import Engine
    e0, srcs = pairs
    eng = Engine(0)
    e, s = device_pairs(e0, srcs[0])
    assert bind_pairs(eng, e, s) == 0, eng.lib.mc_last_error(eng.h)
    e64 = [t.double() for t in e0]
    M = [t.double().abs() for t in e0]
    for t, w in enumerate(WEIGHTS):
        for i in range(len(SIZES)):
            s[i].copy_(srcs[t][i])                                  # the same buffers every update, as a model's
            e64[i] = e64[i] + w * (srcs[t][i].double() - e64[i])
            M[i] = torch.maximum(M[i], torch.maximum(srcs[t][i].double().abs(), e64[i].abs()))
        assert eng.lib.mc_ema_update(eng.h, w, stream()) == 0, eng.lib.mc_last_error(eng.h)
    torch.cuda.synchronize()
    for i, n in enumerate(SIZES):
        M[i] = torch.maximum(M[i], e[i].detach().cpu().double().abs())
        check_bound(e[i], e64[i], M[i], len(WEIGHTS), "numel %d" % n)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(s, srcs[-1]))     # the sources are only read


def test_weight_one_copies_and_weight_zero_keeps(pairs):
    from hipmonocon.engine import Engine
    e0, srcs = pairs
    eng = Engine(0)
    e, s = device_pairs(e0, srcs[0])
    e[3][0] = -0.0                                                      # a signed zero is a bit pattern too
    keep = [t.clone() for t in e]
    assert bind_pairs(eng, e, s) == 0
    assert eng.lib.mc_ema_update(eng.h, 0.0, stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(e, keep))
    assert eng.lib.mc_ema_update(eng.h, 1.0, stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(e, s))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(s, srcs[0]))


# ------------------------------------------------------------------------------------------------ 2. fused == stand-alone
SHAPES = [(64, 32, 3, 3), (131,), (1,), (70000,), (10, 64), (37,), (5,)]
NO_GRAD = 4                 # index of the parameter that never gets a gradient
MISALIGNED_EMA = 5          # index of the parameter whose average starts one float into its storage


class Net(torch.nn.Module):
    def __init__(self, values):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(v.clone().cuda()) for v in values])
        self.register_buffer("running_mean", torch.zeros(CHUNK + 9, device="cuda"))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long, device="cuda"))


def make_side(values, loose_value):
    """a model, a parameter outside it (stepped, but without an entry in the average), the fused optimizer over two groups
    -- a plain class and an amsgrad one with its own lr -- with the clip active, and the model's average"""
    from solver import AdamW, ModelEMA
    net = Net(values)
    loose = torch.nn.Parameter(loose_value.clone().cuda())
    params = list(net.w)
    opt = AdamW([dict(params=params[0::2] + [loose]), dict(params=params[1::2], lr=3e-3, amsgrad=True, betas=(0.8, 0.95))],
                lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, max_grad_norm=5.0)
    ema = ModelEMA(net, decay=0.9, warmup=True)
    k = "w.%d" % MISALIGNED_EMA
    ema.tensors[k] = misaligned(ema.tensors[k])
    return net, loose, opt, ema


def test_fused_equals_standalone_bit_for_bit():
    gen = torch.Generator().manual_seed(5)
    values = [torch.randn(s, generator=gen) for s in SHAPES]
    loose_value = torch.randn(4099, generator=gen)
    grads = [[torch.randn(s, generator=gen) * 3 for s in SHAPES + [(4099,)]] for _ in range(3)]
    stats = [torch.randn(CHUNK + 9, generator=gen) for _ in range(3)]
    A, B = make_side(values, loose_value), make_side(values, loose_value)
    A[2].set_ema(A[3])
    sentinel = torch.full((4099 + 8,), 7.25, device="cuda")           # where an average of the loose parameter would live
    assert A[3].entries_of([A[1]]) == [None]
    assert A[3].entries_of(list(A[0].w))[MISALIGNED_EMA].data_ptr() % 16 == 4
    for t in range(3):
        for net, loose, opt, ema in (A, B):
            for i, p in enumerate(list(net.w) + [loose]):
                p.grad = None if i == NO_GRAD else grads[t][i].clone().cuda()
            net.running_mean.copy_(stats[t])                        # what a train-mode forward does to the buffers
            net.num_batches_tracked.add_(1)
        A[2].step()                                                 # the average inside the AdamW pass + the rest
        B[2].step()
        B[3].update()                                               # the yardstick: everything by mc_ema_update
        assert A[3].updates == B[3].updates == t + 1
    torch.cuda.synchronize()
    assert float(A[2].last_grad_norm) > 5.0                          # the clip was active
    for i, (pa, pb) in enumerate(zip(list(A[0].w) + [A[1]], list(B[0].w) + [B[1]])):
        assert torch.equal(pa, pb), ("param", i)
        sa, sb = A[2].state.get(pa, {}), B[2].state.get(pb, {})
        assert set(sa) == set(sb) and (i == NO_GRAD) == (not sa), i
        for k in sb:
            assert torch.equal(sa[k].cpu(), sb[k].cpu()), (k, i)
        if sb:
            assert ("max_exp_avg_sq" in sb) == (i % 2 == 1 and i < len(SHAPES)), i
        if i != NO_GRAD:
            assert not torch.equal(pa.detach().cpu(), (values + [loose_value])[i]), i
    assert A[3].tensors.keys() == B[3].tensors.keys() and len(A[3].tensors) == len(SHAPES) + 2
    for k in A[3].tensors:
        assert torch.equal(A[3].tensors[k], B[3].tensors[k]), k
    live = A[0].state_dict()
    for k, e in A[3].tensors.items():
        if k == "w.%d" % NO_GRAD:                                   # never stepped: its average is its value
            assert torch.equal(e, live[k]), k
        elif e.is_floating_point():                                 # an average, not the live value
            assert not torch.equal(e, live[k]), k
    assert int(A[3].tensors["num_batches_tracked"]) == 3
    assert bool((sentinel == 7.25).all())


# ------------------------------------------------------------------------------------------------ 3, 4. the C entries
class Raw:
    """three tensors with AdamW state and averages, bound through the C ABI"""

    def __init__(self, seed=3):
        from hipmonocon.engine import Engine
        gen = torch.Generator().manual_seed(seed)
        self.eng = Engine(0)
        self.n = 3
        shapes = [(CHUNK + 5,), (131,), (16, 8)]
        self.p = [torch.randn(s, generator=gen).cuda() for s in shapes]
        self.g = [(torch.randn(s, generator=gen) * 3).cuda() for s in shapes]
        self.m = [(torch.randn(s, generator=gen) * 0.1).cuda() for s in shapes]
        self.v = [torch.rand(s, generator=gen).cuda() for s in shapes]
        self.x = [torch.rand(s, generator=gen).cuda() for s in shapes]
        self.e = [torch.randn(s, generator=gen).cuda() for s in shapes]
        self.numel = (C.c_int64 * self.n)(*[t.numel() for t in self.p])

    def all(self):
        return self.p + self.g + self.m + self.v + self.x + self.e

    def bind(self):
        return self.eng.lib.mc_optim_bind_classes(self.eng.h, self.n, ptr_array(self.p), ptr_array(self.g), ptr_array(self.m),
                                                  ptr_array(self.v), ptr_array(self.x), self.numel, (C.c_int * 3)(0, 1, 0))

    def bind_ema(self, e=None, n=None):
        e = self.e if e is None else e
        return self.eng.lib.mc_optim_bind_ema(self.eng.h, len(e) if n is None else n, ptr_array(e))

    def classes(self):
        from hipmonocon import lib as L
        return (L.OptimClass * 2)((1e-3, 0.9, 0.99, 1e-8, 1e-2, 2, 0, 0), (3e-3, 0.8, 0.95, 1e-6, 0.0, 5, 1, 0))

    def step(self):
        return self.eng.lib.mc_clip_adamw_step_classes(self.eng.h, self.classes(), 2, 5.0, 2.0, None, stream())

    def ema_step(self, w):
        return self.eng.lib.mc_clip_adamw_ema_step_classes(self.eng.h, self.classes(), 2, 5.0, 2.0, w, None, stream())

    def err(self):
        return self.eng.lib.mc_last_error(self.eng.h).decode()


def test_weight_zero_is_the_old_entry():
    a, b = Raw(), Raw()
    start = [t.clone() for t in a.all()]
    assert a.bind() == 0 and a.step() == 0
    assert b.bind() == 0 and b.bind_ema() == 0 and b.ema_step(0.0) == 0, b.err()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a.all(), b.all()))
    assert all(torch.equal(x, y) for x, y in zip(b.e, start[-3:]))         # weight 0: the averages keep every bit
    assert not any(torch.equal(x, y) for x, y in zip(b.p, start[:3]))      # ... and the step did run
    # the same entry with a weight, and with one NULL entry: the other two follow the new parameters
    c = Raw()
    assert c.bind() == 0 and c.bind_ema([c.e[0], None, c.e[2]]) == 0 and c.ema_step(0.25) == 0, c.err()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(c.all()[:15], a.all()[:15]))
    assert torch.equal(c.e[1], start[-2])
    for i in (0, 2):
        e64 = start[-3 + i].double() + 0.25 * (c.p[i].double() - start[-3 + i].double())
        M = torch.maximum(torch.maximum(start[-3 + i].abs(), c.p[i].abs()), c.e[i].abs()).cpu().double()
        check_bound(c.e[i], e64.cpu(), M, 1, "fused, tensor %d" % i)
    # a new optimizer binding drops the averages: the fused entry is the plain one again
    assert c.bind() == 0 and c.ema_step(0.25) == 0
    assert a.step() == 0
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(c.p + c.m + c.v + c.x, a.p + a.m + a.v + a.x))
    assert torch.equal(c.e[1], start[-2])


def test_argument_checks_fail_before_anything_is_launched():
    r = Raw()
    keep = [t.clone() for t in r.all()]
    assert r.bind_ema() != 0 and "bind" in r.err()                          # no optimizer table bound yet
    assert r.bind() == 0
    assert r.bind_ema(r.e[:2]) != 0 and "2" in r.err() and "3" in r.err()   # n differs from the table's size
    assert r.bind_ema([r.e[0], r.p[1], r.e[2]]) != 0 and "alias" in r.err()     # an average that is its parameter
    assert r.bind_ema([r.e[0], r.e[1], r.p[2][2:]]) != 0 and "alias" in r.err()     # ... or overlaps it
    assert r.bind_ema() == 0, r.err()
    for bad in (float("nan"), -0.1, 1.5):
        assert r.ema_step(bad) != 0 and "ema_weight" in r.err(), bad
    # the stand-alone table
    assert r.eng.lib.mc_ema_update(r.eng.h, 0.5, stream()) != 0 and "mc_ema_bind" in r.err()
    numel = r.numel
    assert r.eng.lib.mc_ema_bind(r.eng.h, 3, ptr_array(r.e), ptr_array([r.p[0], r.e[1], r.p[2]]), numel) != 0 and "alias" in r.err()
    assert r.eng.lib.mc_ema_update(r.eng.h, 0.5, stream()) != 0             # a failed bind leaves nothing bound
    assert r.eng.lib.mc_ema_bind(r.eng.h, 3, ptr_array(r.e), ptr_array(r.p), numel) == 0, r.err()
    for bad in (float("nan"), -0.1, 1.5):
        assert r.eng.lib.mc_ema_update(r.eng.h, bad, stream()) != 0 and "ema_weight" in r.err(), bad
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(r.all(), keep))           # parameters, state and averages keep every bit
    # and through Python: an average that shares its storage with the model is refused by the bind
    from hipmonocon.lib import MonoconHipError
    from solver import ModelEMA
    net = Net([torch.ones(8)])
    ema = ModelEMA(net)
    ema.tensors["w.0"] = net.w[0].detach()
    with pytest.raises(MonoconHipError, match="alias"):
        ema.update()
    assert ema.updates == 0


# ------------------------------------------------------------------------------------------------ 5. detector level
def to_cuda(batch):
    d = dict(batch)
    d["img"] = batch["img"].cuda()
    d["label"] = {k: v.cuda() for k, v in batch["label"].items()}
    return d


def snapshot(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_detector_average_follows_three_train_steps(golden_sd, monkeypatch):
    from conftest import GOLDEN_SEED
    from hipmonocon import synth
    from model import MonoConDetector
    from solver import AdamW, ModelEMA
    monkeypatch.setenv("MONOCON_HIP_AUTOTUNE", "0")     # two detectors are compared bit for bit: the same tilings in both

    def detector(sd):
        m = MonoConDetector(34, pretrained_backbone=False)
        m.load_state_dict(sd, strict=True)
        return m.cuda()

    m = detector(golden_sd).train()
    batch = to_cuda(synth.make_batch(GOLDEN_SEED + 9, 2, 96, 160))
    opt = AdamW(m.parameters(), lr=2.25e-4, weight_decay=1e-5, betas=(0.95, 0.99), max_grad_norm=35.0)
    ema = ModelEMA(m, decay=0.9998, warmup=True)
    opt.set_ema(ema)
    states = [snapshot(m)]
    T = 3
    for _ in range(T):
        opt.zero_grad()
        _, loss = m(batch)
        sum(loss.values()).backward()
        opt.step()
        states.append(snapshot(m))
    torch.cuda.synchronize()
    assert ema.updates == T
    some_stat_differs = False
    for k, e in ema.tensors.items():
        if not e.is_floating_point():
            assert k.endswith("num_batches_tracked") and int(e) == int(states[-1][k]) == T, k
            continue
        e64 = states[0][k].double()
        M = e64.abs()
        for t in range(T):
            x = states[t + 1][k].double()
            e64 = e64 + (1.0 - ema.decay_at(t)) * (x - e64)
            M = torch.maximum(M, torch.maximum(x.abs(), e64.abs()))
        err = (e.double() - e64).abs()
        assert bool((err <= T * EPS * torch.maximum(M, e.double().abs())).all()), (k, float(err.max()))
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert e.data_ptr() != states[-1][k].data_ptr()
            some_stat_differs |= not torch.equal(e, states[-1][k])
    assert some_stat_differs                            # the buffers are averaged, neither aliased nor copied
    # evaluation on the averaged weights, and back
    m.eval()
    img = {"img": batch["img"]}
    with torch.no_grad():
        out_live = {k: v.clone() for k, v in m(dict(img)).items()}     # (the packed-weight cache now holds the live weights)
        before = snapshot(m)
        with ema.applied(m):
            out_ema = {k: v.clone() for k, v in m(dict(img)).items()}
            assert all(torch.equal(v, ema.tensors[k]) for k, v in m.state_dict().items())
        fresh = detector({k: v.cpu() for k, v in ema.state_dict()["tensors"].items()}).eval()
        out_fresh = fresh(dict(img))
        for k in out_ema:
            assert torch.equal(out_ema[k], out_fresh[k]), k
        assert any(not torch.equal(out_ema[k], out_live[k]) for k in out_ema)
        after = snapshot(m)
        assert all(torch.equal(after[k], before[k]) for k in before)
        out_after = m(dict(img))
        for k in out_live:                                             # a stale packed-weight cache fails here, not above
            assert torch.equal(out_after[k], out_live[k]), k


# ------------------------------------------------------------------------------------------------ 6. engine
def engine_cfg(out_dir, ema):
    from utils.engine_utils import get_default_cfg
    cfg = get_default_cfg()
    cfg.set_new_allowed(True)
    cfg.OUTPUT_DIR = str(out_dir)
    cfg.SEED = 3
    cfg.DATA.ROOT = 'synthetic'
    cfg.DATA.SYNTHETIC_LENGTH = 4
    cfg.DATA.SYNTHETIC_HW = [96, 224]
    cfg.DATA.BATCH_SIZE = 2
    cfg.DATA.NUM_WORKERS = 0
    cfg.MODEL.BACKBONE.IMAGENET_PRETRAINED = False
    cfg.SOLVER.OPTIM.NUM_EPOCHS = 2
    cfg.SOLVER.EMA.ENABLE = ema
    cfg.SOLVER.EMA.DECAY = 0.99
    cfg.PERIOD.EVAL_PERIOD = 0
    cfg.PERIOD.LOG_PERIOD = 1
    return cfg


def test_engine_trains_evaluates_and_checkpoints_the_average(tmp_path):
    from engine.monocon_engine import MonoconEngine
    from solver import ModelEMA
    from utils.engine_utils import set_random_seed
    set_random_seed(3)
    on, off = os.path.join(tmp_path, "on"), os.path.join(tmp_path, "off")
    os.makedirs(on), os.makedirs(off)
    eng = MonoconEngine(engine_cfg(on, True))
    assert isinstance(eng.ema, ModelEMA) and eng.optimizer._ema is eng.ema
    assert (eng.ema.decay, eng.ema.warmup, eng.ema.updates) == (0.99, True, 0)
    eng.train_one_epoch()
    torch.cuda.synchronize()
    assert eng.ema.updates == 2 and len(eng.entire_losses) == 2
    live = snapshot(eng.model)
    assert any(not torch.equal(live[k], e) for k, e in eng.ema.tensors.items())
    ev = eng.evaluate()
    assert ev['num_results'] == 1.0
    after = snapshot(eng.model)
    assert all(torch.equal(after[k], live[k]) for k in live)               # evaluate() put the live weights back
    eng.save_checkpoint(post_fix='t')
    path = os.path.join(on, 'checkpoints', 'epoch_001_t.pth')
    d = torch.load(path, weights_only=False)
    assert set(d['state_dict']) == {'model', 'optimizer', 'scheduler', 'ema'} and 'ema' not in d['engine_attrs']
    assert set(d['state_dict']['ema']) == {'tensors', 'updates', 'decay', 'warmup'}
    eng2 = MonoconEngine(engine_cfg(on, True))                              # auto-resume finds the file
    assert eng2.epochs == 2 and eng2.ema.updates == 2 and eng2.optimizer._ema is eng2.ema
    for k, e in eng.ema.tensors.items():
        assert e.dtype == eng2.ema.tensors[k].dtype and torch.equal(e, eng2.ema.tensors[k]) and eng2.ema.tensors[k].is_cuda, k
    # a run without the average writes the reference's three keys; an EMA-enabled engine starts its average from them
    eng3 = MonoconEngine(engine_cfg(off, False))
    assert eng3.ema is None and eng3.optimizer._ema is None
    eng3.save_checkpoint(post_fix='t', save_after_update=False)
    d = torch.load(os.path.join(off, 'checkpoints', 'epoch_001_t.pth'), weights_only=False)
    assert set(d['state_dict']) == {'model', 'optimizer', 'scheduler'} and 'ema' not in d['engine_attrs']
    eng2.load_checkpoint(os.path.join(off, 'checkpoints', 'epoch_001_t.pth'))
    plain = snapshot(eng3.model)
    assert eng2.ema.updates == 0
    assert all(torch.equal(eng2.ema.tensors[k], plain[k]) for k in plain)
    assert all(torch.equal(v, plain[k]) for k, v in eng2.model.state_dict().items())
    # the scripts' --use_ema: the averaged weights into a detector, and a clear error for a file without them
    det = eng3.model
    det.load_checkpoint(path, use_ema=True)
    assert all(torch.equal(v, eng.ema.tensors[k]) for k, v in det.state_dict().items())
    with pytest.raises(KeyError, match="no averaged weights"):
        det.load_checkpoint(os.path.join(off, 'checkpoints', 'epoch_001_t.pth'), use_ema=True)
