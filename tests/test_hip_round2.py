"""GPU tests added in round 2: BASELINE's full batch sizes (B=32 at 384x1280), optimizer resume, the stand-alone loss
API of the heads, the train-forward generation guard, label validation, and the data-parallel path on two ranks
(both on device 0 over gloo: the box has one GPU and RCCL refuses a shared device)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_err, grad_rel_l2, GOLDEN_SEED
from hipmonocon import netspec, synth

pytestmark = pytest.mark.gpu


def to_cuda(batch):
    d = dict(batch)
    d["img"] = batch["img"].cuda()
    d["label"] = {k: v.cuda() for k, v in batch["label"].items()}
    return d


def build(sd, train=True):
    from model import MonoConDetector
    m = MonoConDetector(34, pretrained_backbone=False)
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    return m.train() if train else m.eval()


# ------------------------------------------------------------------------------------- BASELINE batch sizes
def test_b32_eval_forward_matches_the_b2_reference_golden(golden_sd):
    """BASELINE configs[1] (B=32, 384x1280, fp32, forward only): the two golden images of fwd_full_eval.npz placed at
    rows 0 / 1 and 30 / 31 of a B=32 batch (other rows: other images) must reproduce the reference's fp64 samples at
    1e-4, and rows 30 / 31 must be bit-identical to rows 0 / 1 (eval mode: batch invariance across plan shapes)."""
    g = load_golden("fwd_full_eval.npz")
    two = synth.make_batch(GOLDEN_SEED + 2, 2, 384, 1280, with_labels=False)["img"]
    other = torch.randn((28, 3, 384, 1280), generator=torch.Generator().manual_seed(11))
    imgs = torch.cat([two, other, two]).cuda()
    m = build(golden_sd, train=False)
    pred = m({"img": imgs})
    torch.cuda.synchronize()
    for k, v in pred.items():
        assert v.shape[0] == 32
        assert torch.equal(v[30:32], v[0:2]), k
        s = v[0:2].detach().cpu().reshape(-1)[::97]
        assert rel_err(s, g[k + ".f64sample"]) < 1e-4, (k, rel_err(s, g[k + ".f64sample"]))
        assert bool(torch.isfinite(v).all()), k


def test_b32_train_step_equals_the_b2_step_repeated_16_times(golden_sd):
    """BASELINE configs[2] shape (B=32, 384x1280 train step).  A batch that repeats a B=2 batch 16 times has the same
    BatchNorm batch statistics, the same per-object losses and 16x the object count, so every loss equals the B=2
    loss and every gradient tensor equals the B=2 gradient (different summation trees: tolerance 2e-4 on the losses,
    1e-3 relative L2 on the flat gradient); run twice: bit-identical (deterministic reductions at full size)."""
    b2 = synth.make_batch(GOLDEN_SEED + 21, 2, 384, 1280)
    m2 = build(golden_sd)
    _, l2 = m2(to_cuda(b2))
    sum(l2.values()).backward()
    g2 = torch.cat([p.grad.flatten() for p in m2.parameters() if p.grad is not None]).clone()
    l2 = {k: float(v.detach()) for k, v in l2.items()}
    del m2
    b32 = {"img": b2["img"].repeat(16, 1, 1, 1).cuda(), "label": {k: v.repeat(16, *([1] * (v.dim() - 1))).cuda() for k, v in b2["label"].items()},
           "img_metas": {"pad_shape": [(384, 1280)] * 32}}
    outs = []
    for _ in range(2):
        m = build(golden_sd)
        _, l32 = m(b32)
        sum(l32.values()).backward()
        torch.cuda.synchronize()
        outs.append((torch.stack([v.detach() for v in l32.values()]).clone(),
                     torch.cat([p.grad.flatten() for p in m.parameters() if p.grad is not None]).clone()))
        for k, v in l32.items():
            assert abs(float(v.detach()) - l2[k]) <= 2e-4 * abs(l2[k]) + 1e-7, (k, float(v.detach()), l2[k])
        del m
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    g32 = outs[0][1]
    assert bool(torch.isfinite(g32).all())
    rel = float((g32.double() - g2.double()).norm() / g2.double().norm())
    assert rel < 1e-3, rel


# ------------------------------------------------------------------------------------- optimizer resume
def test_fused_adamw_resume_matches_an_uninterrupted_run(golden_sd, tmp_path):
    """reference engine/base_engine.py:155-219: model + optimizer + scheduler state_dicts.  Three steps, checkpoint,
    rebuild everything from the checkpoint, two more steps == five uninterrupted steps, bit for bit (same kernels,
    same bias-correction step, same moments); the optimizer state carries torch.optim.AdamW's per-parameter keys."""
    from solver import AdamW, CyclicScheduler
    batches = [to_cuda(synth.make_batch(300 + i, 2, 96, 160)) for i in range(5)]

    def make():
        m = build(golden_sd)
        opt = AdamW(m.parameters(), lr=2.25e-4, weight_decay=1e-5, betas=(0.95, 0.99), max_grad_norm=35.0)
        return m, opt, CyclicScheduler(opt, total_steps=50)

    def run(m, opt, sch, bs):
        for b in bs:
            opt.zero_grad()
            _, loss = m(b)
            sum(loss.values()).backward()
            opt.step()
            sch.step()

    ma, oa, sa = make()
    run(ma, oa, sa, batches)
    mb, ob, sb = make()
    run(mb, ob, sb, batches[:3])
    st = ob.state_dict()
    some = next(iter(st["state"].values()))
    assert set(some) == {"step", "exp_avg", "exp_avg_sq"} and float(some["step"]) == 3.0
    path = os.path.join(tmp_path, "ck.pth")
    torch.save({"model": mb.state_dict(), "optimizer": st, "scheduler": sb.state_dict()}, path)
    del mb, ob, sb
    ck = torch.load(path, map_location="cpu", weights_only=False)
    mc, oc, sc = make()
    mc.load_state_dict(ck["model"])
    oc.load_state_dict(ck["optimizer"])
    sc.load_state_dict(ck["scheduler"])
    assert sc._step_count == 4
    run(mc, oc, sc, batches[3:])
    for (n, pa), (_, pc) in zip(ma.named_parameters(), mc.named_parameters()):
        assert torch.equal(pa, pc), n
    for (n, ba), (_, bc) in zip(ma.named_buffers(), mc.named_buffers()):
        assert torch.equal(ba, bc), n
    # a load AFTER a step must re-bind the kernels to the loaded moment tensors (they are new allocations)
    md, od, sd_ = make()
    run(md, od, sd_, batches[:1])
    md.load_state_dict(ck["model"])
    od.load_state_dict(ck["optimizer"])
    sd_.load_state_dict(ck["scheduler"])
    run(md, od, sd_, batches[3:])
    for (n, pa), (_, pd) in zip(ma.named_parameters(), md.named_parameters()):
        assert torch.equal(pa, pd), n


def test_fused_adamw_resume_vs_torch_adamw(golden_sd):
    """warm moments + step restored: the first update after a load equals torch.optim.AdamW's (the round-1 bug made
    it ~2x too large by restarting the bias correction at step 1)."""
    from solver import AdamW
    torch.manual_seed(3)
    shapes = [(64, 32, 3, 3), (128,), (70001,)]
    base = [torch.randn(s) for s in shapes]
    pa = [torch.nn.Parameter(b.clone().cuda()) for b in base]
    pb = [torch.nn.Parameter(b.clone()) for b in base]
    oa = AdamW(pa, lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.99))
    ob = torch.optim.AdamW(pb, lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.99))
    def step(it):
        for p, q, s in zip(pa, pb, shapes):
            gr = torch.randn(s, generator=torch.Generator().manual_seed(100 + it))
            p.grad, q.grad = gr.cuda(), gr.clone()
        oa.step(); ob.step()
    for it in range(4):
        step(it)
    pa2 = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa2 = AdamW(pa2, lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.99))
    oa2.load_state_dict(oa.state_dict())
    pa, oa = pa2, oa2
    for it in range(4, 6):
        step(it)
        for p, q in zip(pa, pb):
            assert rel_err(p.detach().cpu(), q.detach()) < 2e-6


# ------------------------------------------------------------------------------------- head API
def test_heads_get_losses_standalone_with_autograd(golden_sd):
    """MonoConDenseHeads._get_losses(pred_dict, target_dict) (reference monocon_heads.py:203-310): loss values and
    the gradient with respect to the PREDICTION maps vs torch autograd through the oracle's loss code."""
    from oracle import monocon_oracle as O
    batch = synth.make_batch(GOLDEN_SEED + 9, 2, 192, 384)
    with torch.no_grad():
        preds, Tref, _, _ = O.train_forward(golden_sd, batch)
    leaf = {k: v.clone().requires_grad_(True) for k, v in preds.items()}
    Lref = O.losses(leaf, Tref)
    w = torch.tensor([1.0, 0.5, 2.0, 1.5, 1.0, 0.7, 1.0, 3.0, 1.0, 0.25])
    sum(w[i] * v for i, v in enumerate(Lref.values())).backward()
    m = build(golden_sd)
    cl = {k: v.clone().cuda().requires_grad_(True) for k, v in preds.items()}
    T = {k: v.cuda() for k, v in Tref.items()}
    L = m.head._get_losses(cl, T)
    assert list(L.keys()) == list(netspec.LOSS_KEYS)
    for k, v in L.items():
        assert v.dim() == 0 and v.requires_grad
        assert abs(float(v.detach()) - float(Lref[k])) <= 1e-4 * abs(float(Lref[k])) + 1e-6, k
    sum(w[i].cuda() * v for i, v in enumerate(L.values())).backward()
    for k in preds:
        assert rel_err(cl[k].grad.cpu(), leaf[k].grad) < 2e-4, (k, rel_err(cl[k].grad.cpu(), leaf[k].grad))


def test_heads_forward_train_standalone(cond_sd):
    """MonoConDenseHeads.forward_train(feat, data_dict) (reference monocon_heads.py:150-157) on its own: the ten
    losses, the gradient with respect to ``feat`` and the gradients of all head parameters vs torch autograd through
    the oracle's head (fp64), and the AttnBN running buffers ticked as the reference's."""
    from oracle import monocon_oracle as O
    from model import MonoConDenseHeads
    B, H, W = 4, 64, 128
    batch = synth.make_conditioned_batch(812, B, H, W)
    feat = torch.from_numpy(synth.normalish(5, "feat", (B, 64, H // 4, W // 4)).astype(np.float32)).abs()   # post-ReLU-like
    # oracle in float64: head only
    sd64 = {k: (v.double().clone() if v.dtype == torch.float32 else v.clone()) for k, v in cond_sd.items()}
    for k, v in sd64.items():
        if k.startswith("head.") and v.dtype == torch.float64 and "running" not in k:
            v.requires_grad_(True)
    f64 = feat.double().clone().requires_grad_(True)
    cx = O._Ctx(sd64, True)
    preds = O.head_predictions(cx, f64)
    T = O.make_targets(batch["label"], (H, W), tuple(f64.shape))
    L = O.losses(preds, T)
    sum(L.values()).backward()
    heads = MonoConDenseHeads(test_config=None)
    heads.load_state_dict({k[5:]: v for k, v in cond_sd.items() if k.startswith("head.")}, strict=True)
    heads = heads.cuda().train()
    fc = feat.clone().cuda().requires_grad_(True)
    data = {"label": {k: v.cuda() for k, v in batch["label"].items()}, "img_metas": batch["img_metas"]}
    pd, ld = heads.forward_train(fc, data)
    assert list(ld.keys()) == list(netspec.LOSS_KEYS) and set(pd) == {k for k, _ in netspec.PRED_KEYS}
    for k, v in ld.items():
        assert abs(float(v.detach()) - float(L[k])) <= 1e-4 * abs(float(L[k])) + 1e-7, (k, float(v.detach()), float(L[k]))
    for k, v in pd.items():
        assert rel_err(v.detach().cpu(), preds[k].detach()) < 1e-4, k
    sum(ld.values()).backward()
    e = float((fc.grad.cpu().double() - f64.grad).norm() / f64.grad.norm())
    assert e < 1e-3, e
    for n, p in heads.named_parameters():
        ref = sd64["head." + n].grad
        assert p.grad is not None and ref is not None, n
        scale = max(float(ref.norm()), 1e-12)
        assert float((p.grad.cpu().double() - ref).norm()) / scale < 2e-3, (n, float((p.grad.cpu().double() - ref).norm()) / scale)
    sdh = heads.state_dict()
    for k, v in cx.new_buffers.items():
        if k.startswith("head.") and not k.endswith("num_batches_tracked"):
            assert rel_err(sdh[k[5:]].cpu(), v) < 1e-4, k
    with pytest.raises(Exception):
        heads.forward_train(fc[:, :32], data)


def test_query_workspace_predicts_what_the_plans_allocate(golden_sd):
    """mc_query_workspace: the dry run of the plan builders reports exactly the bytes the real build
    allocates afterwards -- inference plan and train plan -- and allocates nothing itself."""
    from hipmonocon.train import _binding
    m = build(golden_sd, train=False)
    eng = m._engine()
    base = eng.workspace_bytes()
    q_inf = eng.query_workspace(2, 64, 128, "infer")
    assert q_inf > 0 and eng.workspace_bytes() == base
    m({"img": torch.zeros(2, 3, 64, 128, device="cuda")})
    assert eng.workspace_bytes() - base == q_inf
    assert eng.query_workspace(2, 64, 128, "infer") == q_inf            # built plan: same answer
    m.train()
    tb = _binding(m)
    eng = m._rt.get(tb.state(m))                                         # binds the "#grad" buffers too
    base = eng.workspace_bytes()
    q_tr = eng.query_workspace(3, 64, 128, "train")
    assert q_tr > q_inf and eng.workspace_bytes() == base
    _, loss = m(to_cuda(synth.make_batch(9, 3, 64, 128)))
    assert eng.workspace_bytes() - base == q_tr
    sum(loss.values()).backward()
    assert eng.workspace_bytes() - base == q_tr
    # full size, without building anything: the number DESIGN.md quotes for B=32
    q32 = eng.query_workspace(32, 384, 1280, "train")
    assert 26e9 < q32 < 34e9, q32      # (45.3 GB before round 3: dY in place over dZ, recycled gradient maps)


def test_train_plan_rejects_a_grad_buffer_of_the_wrong_size(golden_sd):
    """the train plan checks every tensor it binds -- "#grad" buffers included -- for dtype and size: a gradient buffer one
    element too large (which would keep an unchecked build in bounds) fails the build with an error naming its key"""
    from hipmonocon.engine import Engine
    from hipmonocon.lib import MonoconHipError
    from hipmonocon.train import _binding
    m = build(golden_sd)
    st = _binding(m).state(m)
    key = "backbone.level3.tree1.tree2.conv1.weight#grad"
    st[key] = torch.zeros(st[key].numel() + 1, device="cuda")
    eng = Engine(0)
    eng.bind_state(st)
    with pytest.raises(MonoconHipError, match=key):
        eng.build_train_plan(2, 64, 128)


def test_recycled_gradient_buffers_do_not_change_a_bit(golden_sd, monkeypatch):
    """round 3: dY in place over dZ + gradient maps from a pool (a buffer last read by the weight-gradient stream is waited for
    before its next first write).  Same kernels, other addresses: losses and every gradient must be bit-identical to the plan
    with one private buffer per map (MONOCON_HIP_GRAD_POOL=0), also with immediate recycling (..._COOL=0, the tightest
    cross-stream coupling), over several steps; and the pooled plan must be the smaller one."""
    batch = to_cuda(synth.make_batch(GOLDEN_SEED + 41, 3, 96, 160))

    def run(pool, cool):
        monkeypatch.setenv("MONOCON_HIP_GRAD_POOL", pool)
        monkeypatch.setenv("MONOCON_HIP_GRAD_POOL_COOL", cool)
        m = build(golden_sd)
        outs = []
        for _ in range(3):
            for p in m.parameters():
                p.grad = None
            _, loss = m(batch)
            sum(loss.values()).backward()
            torch.cuda.synchronize()
            outs.append((torch.stack([v.detach() for v in loss.values()]).clone(),
                         torch.cat([p.grad.flatten() for p in m.parameters() if p.grad is not None]).clone()))
        return outs, m._rt.engine.workspace_bytes()
    private, ws_private = run("0", "0")
    for cool in ("0", "2"):
        pooled, ws_pooled = run("1", cool)
        for (la, ga), (lb, gb) in zip(private, pooled):
            assert torch.equal(la, lb) and torch.equal(ga, gb), cool
        assert ws_pooled < ws_private


# ------------------------------------------------------------------------------------- guards
def test_backward_of_a_stale_forward_raises(golden_sd):
    from hipmonocon.lib import MonoconHipError
    m = build(golden_sd)
    b = to_cuda(synth.make_batch(5, 2, 64, 128))
    _, l1 = m(b)
    _, l2 = m(b)
    with pytest.raises(MonoconHipError, match="saved activations"):
        sum(l1.values()).backward()
    sum(l2.values()).backward()          # the latest forward is fine
    assert all(p.grad is not None for n, p in m.named_parameters() if n not in netspec.DEAD_PARAMS)


def test_out_of_map_labels_raise_like_the_reference(golden_sd):
    """reference utils/target_generator.py:70-75 indexes the heat-map with the truncated box centre and the class id:
    a centre outside the map / an unknown class is an IndexError there, and here (before any launch)."""
    m = build(golden_sd)
    b = synth.make_batch(6, 2, 64, 128)
    bad = {k: v.clone() for k, v in b["label"].items()}
    bad["gt_bboxes"][0, 0] = torch.tensor([200.0, 10.0, 260.0, 40.0])      # centre x = 230 > 128
    with pytest.raises(IndexError):
        m(to_cuda({"img": b["img"], "label": bad, "img_metas": b["img_metas"]}))
    bad = {k: v.clone() for k, v in b["label"].items()}
    bad["gt_labels"][1, 0] = 7.0
    with pytest.raises(IndexError):
        m(to_cuda({"img": b["img"], "label": bad, "img_metas": b["img_metas"]}))
    m(to_cuda(b))                                                           # the clean batch still runs


# ------------------------------------------------------------------------------------- data parallel, 2 ranks
_DP_WORKER = r'''
import os, sys, json
sys.path.insert(0, os.path.join(%(repo)r, "monocon-pytorch_amd")); sys.path.insert(0, %(repo)r); sys.path.insert(0, os.path.join(%(repo)r, "tests"))
import numpy as np, torch, torch.distributed as dist
from conftest import load_golden, grad_rel_l2
from hipmonocon import synth, netspec, dist as hdist
from model import MonoConDetector
from solver import AdamW
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
import traceback
def _excepthook(t, v, tb):
    open(os.path.join(%(tmp)r, "rank%%d.err" %% rank), "w").write("".join(traceback.format_exception(t, v, tb)))
    sys.__excepthook__(t, v, tb)
sys.excepthook = _excepthook
torch.cuda.set_device(0)
dist.init_process_group("gloo")
g = load_golden("dp_shards.npz")
stats = load_golden("bn_calib_seed7.npz")
sd = synth.make_conditioned_state_dict(7, bn_stats={k: stats[k] for k in stats.files})
B, H, W = (int(x) for x in g["shape"])
gb = synth.make_conditioned_batch(int(g["seed"]), B, H, W)
sb = hdist.shard_batch(gb, rank, world)
torch.manual_seed(100 + rank)                         # different RNG state per rank: the replicas must still agree
m = MonoConDetector(34, pretrained_backbone=False)
if rank == 0:
    m.load_state_dict(sd, strict=True)                # rank 1 keeps its own random init until the broadcast
m = m.cuda().train()
n_sync = hdist.sync_module_state(m)
assert n_sync == 449
cs = torch.tensor([hdist.state_checksum(m)], dtype=torch.float64)
lst = [torch.zeros_like(cs) for _ in range(world)]
dist.all_gather(lst, cs)
assert all(float(x) == float(lst[0]) for x in lst), lst
batch = {"img": sb["img"].cuda(), "label": {k: v.cuda() for k, v in sb["label"].items()}, "img_metas": sb["img_metas"]}
opt = AdamW(m.parameters(), lr=2.25e-4, weight_decay=1e-5, betas=(0.95, 0.99), max_grad_norm=35.0)
opt.zero_grad()
_, loss = m(batch)
for k, v in loss.items():
    ref = float(g["w%%d.r%%d.f64.%%s" %% (world, rank, k)])
    assert abs(float(v.detach()) - ref) <= 1e-4 * abs(ref) + 1e-7, (rank, k, float(v.detach()), ref)
sum(loss.values()).backward()                         # includes the all-reduce(mean) of the flat gradient buffer
worst = 0.0
for n, p in m.named_parameters():
    if n in netspec.DEAD_PARAMS:
        assert p.grad is None
        continue
    e = grad_rel_l2(p.grad, g["w%%d.g64.%%s" %% (world, n)], g["w%%d.gnorm64.%%s" %% (world, n)], p.numel())
    # the shards are not selected flip-free (B=2 / B=4 sub-batches): a flipped ReLU decision shifts a tensor by up to
    # ~1e-2, a wrong reduction (sum instead of mean, a missing shard) by 0.3 .. 1
    # (world 4 = shards of 2 images: BatchNorm over two samples inside AttnBN is the worst-conditioned case there is)
    bound = 4.0 * float(g["w%%d.gerr32.%%s" %% (world, n)]) + (2e-2 if world == 2 else 6e-2)
    assert e <= bound, (rank, n, e, bound)
    worst = max(worst, e)
opt.step()
flat = torch.cat([p.detach().flatten() for p in m.parameters()]).cpu()
lst = [torch.zeros_like(flat) for _ in range(world)]
dist.all_gather(lst, flat)
assert all(torch.equal(x, lst[0]) for x in lst), "parameters differ across ranks after the optimizer step"
print("DP_OK rank %%d worst grad err %%.2e" %% (rank, worst), flush=True)
dist.barrier()
dist.destroy_process_group()
'''


@pytest.mark.parametrize("world", [2, 4])
def test_data_parallel_ranks_on_one_device_over_gloo(tmp_path, world):
    """SURVEY 8e / 8c golden (8): N ranks (all on device 0, gloo) run MonoConDetector forward + backward on their
    shard of a global batch of 8; after the in-backward all-reduce every rank's gradients equal the mean of the
    reference's per-shard fp64 gradients (tests/golden/dp_shards.npz), rank 1 starts from its own random init and is
    overwritten by the rank-0 broadcast, and after the fused optimizer step the parameters are bit-identical on all
    ranks."""
    script = os.path.join(tmp_path, "dp_worker.py")
    open(script, "w").write(_DP_WORKER % {"repo": REPO, "tmp": str(tmp_path)})
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONDONTWRITEBYTECODE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), script]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    errs = "".join(open(os.path.join(tmp_path, f)).read() for f in sorted(os.listdir(tmp_path)) if f.endswith(".err"))
    assert r.returncode == 0, "worker failure:\n" + errs[-4000:] + "\n---- launcher stderr tail ----\n" + r.stderr[-1500:]
    assert r.stdout.count("DP_OK") == world, r.stdout[-2000:]


def test_bench_multi_rank_path_end_to_end(tmp_path):
    """the command the driver's scaling run uses, `python bench.py --gpus N ...`, on a 1-GPU box: two ranks on device 0
    over gloo (MONOCON_BENCH_BACKEND, a control-flow hook -- not a measurement).  Exercises the self-launch under
    torch.distributed.run, the rank-0 state broadcast, the in-backward gradient all-reduce, the barrier-bracketed
    timing with the max over ranks, and the single JSON line of rank 0."""
    import json
    env = dict(os.environ, MONOCON_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONDONTWRITEBYTECODE="1")
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "4",
           "--height", "64", "--width", "128", "--full", "--forward-steps", "2", "--no-cpu-baseline", "--no-extra-modes",
           # (its verbose report must not land on the default gpurun_out/bench_full.json: round 4 copied a report overwritten
           #  by this test into profiles/ as the headline run's)
           "--full-json", os.path.join(str(tmp_path), "bench_full.json")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["world_size"] == 2 and d["collective_backend"] == "gloo"
    assert d["scaling"] == "weak" and d["config"]["global_batch"] == 8 and d["config"]["parallelism"] == "dp2"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 2
    assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) <= 0.02 * d["value"]      # whole-job images / second
    assert d["roofline"]["bound"] == "mfma" and d["roofline"]["achieved"] > 0


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """`python bench.py` without --full times the headline train step and nothing else: one JSON line with the contract
    keys and none of the --full legs, and --dump-outputs still writes the outputs of the last timed step"""
    import json
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    dump = os.path.join(str(tmp_path), "dump")
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "4",
           "--height", "64", "--width", "128", "--dump-outputs", dump, "--full-json", os.path.join(str(tmp_path), "report.json")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["dtype"].startswith("f32 (")
    assert abs(d["value"] - 4 / (d["ms_per_step"] * 1e-3)) <= 0.02 * d["value"]
    for k in ("roofline", "forward_only", "modes", "realistic_loop", "engine_feed", "engine_feed_kitti", "input_feed",
              "decode_only", "kitti_eval_overlaps", "cpu_baseline"):
        assert k not in d, k
    names = {f[:-4] for f in os.listdir(dump) if f.endswith(".npy")}
    assert names == set(netspec.LOSS_KEYS) | {k for k, _ in netspec.PRED_KEYS} | {"loss_total", "grad_sample", "state_sample"}
    assert all(np.isfinite(np.load(os.path.join(dump, n + ".npy"))).all() for n in names)


# ------------------------------------------------------------------------------------- round 3: advisor findings
def test_loss_dict_entries_can_be_weighted_in_place(golden_sd):
    """the ten losses are independent 0-dim tensors (not views of one buffer): `loss_dict[k] *= w` -- legal on the
    reference's loss_dict -- works, and the backward sees the weight"""
    batch = to_cuda(synth.make_batch(GOLDEN_SEED + 41, 2, 64, 128))
    m = build(golden_sd)
    _, loss = m(batch)
    sum(loss.values()).backward()
    g1 = torch.cat([p.grad.flatten() for p in m.parameters() if p.grad is not None]).clone()
    m2 = build(golden_sd)
    _, loss2 = m2(batch)
    for k in loss2:
        loss2[k] *= 2.0
    sum(loss2.values()).backward()
    g2 = torch.cat([p.grad.flatten() for p in m2.parameters() if p.grad is not None])
    assert float((g2 - 2.0 * g1).abs().max()) <= 1e-6 * float(g1.abs().max()) + 1e-12


def test_heads_only_plan_rules(golden_sd):
    """mc_backward refuses a heads-only plan (mc_head_backward is its entry), and a heads-only backward whose feat does
    not require grad skips the data gradient into feat yet leaves the same parameter gradients"""
    import ctypes as C
    from model import MonoConDenseHeads
    from hipmonocon import lib as hlib
    heads = MonoConDenseHeads(in_ch=64).cuda().train()
    heads.load_state_dict({k[5:]: v for k, v in golden_sd.items() if k.startswith("head.")}, strict=True)
    batch = to_cuda(synth.make_batch(GOLDEN_SEED + 42, 2, 64, 128))
    feat = torch.randn(2, 64, 16, 32, device="cuda")
    grads = []
    for rg in (True, False):
        for p in heads.parameters():
            p.grad = None
        f = feat.clone().requires_grad_(rg)
        _, loss = heads.forward_train(f, batch)
        sum(loss.values()).backward()
        grads.append(torch.cat([p.grad.flatten() for p in heads.parameters()]).clone())
        assert (f.grad is not None) == rg
    # (the second forward starts from moved running statistics, whose mean is the shift of the variance sums: round-off only)
    assert float((grads[0] - grads[1]).abs().max()) <= 1e-4 * float(grads[0].abs().max())
    eng = heads._rt.engine
    g = torch.ones(10, device="cuda")
    rc = eng.lib.mc_backward(eng.h, C.c_void_p(g.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and b"heads-only" in eng.lib.mc_last_error(eng.h)
