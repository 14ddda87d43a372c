"""Every workgroup shape the conv autotuner can pick, in every precision mode, pinned to "the choice never changes a bit".

mc_choose_conv_cfg (csrc/mc_api.hip) times up to twelve candidates per conv signature and keeps the fastest: the six tilings
{1: 128x128, 4: 128x64, 5: 128x64m, 6: 128x32, 7: 64x128, 8: 64x64} (pixels x channels of a workgroup), the wave-specialised
variants (id | 16), the row kernel (32) and the weight-resident kernel (4 | 64).  DESIGN.md section 5 promises that the
accumulation order of an output element does not depend on the shape.  This module forces every eligible shape instead of
waiting for timing noise to select it:

1. op level (mc_op_conv / mc_op_conv_dgrad, `set_conv_cfg`): modes 0 fp32, 1 bf16, 2 bf16x3, 3 f16x2; every case of
   test_hip_ops.py's CONV_CASES / DGRAD_CASES plus the pixel-side edge shapes below; every eligible id bit-identical to the
   automatic choice, which is held to the fp64 reference at the tolerance the project already uses for that op and mode.
2. whole plans through the tune table (`build_train_plan` + `tune_export`, rewritten, `tune_import` on a fresh handle): the
   train step at (2, 96, 160) and the eval forward at (2, 64, 128), every tiling against the 128x32 run, which is held to the
   oracle / the golden.  The table must come back unchanged (a grown table = some launch was tuned instead of dictated).
3. a table naming a tiling whose column tile does not divide the layer's padded column count is refused as a whole, and so
   is every id without an entry in the table of tilings (the retired 2 and 3), by `set_conv_cfg` and `tune_import` alike.

Covered by the whole-plan matrix (checked by test_plan_matrix_covers_every_conv_class and the twin-line assertion of every
run; "BM" = backward-statistics epilogue twins, "LZ" = lazy-source staging, reached with MONOCON_HIP_LAZY_Z=3 /
MONOCON_HIP_LAZY_MIN=0).  The column is (ks, stride) of the table key; 12 / 21 / 22 are the parity classes of the stride-2 data
gradients, 1/1 includes their fourth class:

    precision        3/1            3/2            1/1            12/1, 21/1, 22/1   variants
    fp32             1 4 5 6 7 8    1 4 5 6 7 8    1 4 5 6 7 8    1 4 5 6 7 8        plain, BM; ids 17 21 23 24 (plain launches)
    bf16x3           1 4 5 6 7 8    1 4 5 6 7 8    1 4 5 6 7 8    1 4 5 6 7 8        plain, BM
    f16x2            1 4 5 6 7 8    1 4 5 6 7 8    1 4 5 6 7 8    1 4 5 6 7 8        plain, BM (every map stored at this size); 4 | 64
    f16x2 all-lazy   1 4 5 6 7 8    1 4 5 6 7 8    1 4 5 6 7 8    1 4 5 6 7 8        plain, BM, LZ (16 signatures); 4 | 64

    (measured at 2x96x160 on an MI355X: 55 - 59 signatures per variant, every class of every variant holds a 128-column one,
    so no combination is skipped; a tiling reaches the entries whose padded column count its column tile divides, the others
    run 128x32.  The lazy-source signatures of the all-lazy variant: ten 3/1, four 3/2, two 1/1, 64 to 512 columns.  Left to
    itself the tuner picks only 6, 8 and 24 at this size: every other shape runs here because it is dictated.  The test computes
    the set from the exported table and requires every tiling wherever some column count of the class is divisible, and at
    least two distinct tilings per class.)  BM exists for 3/1 and 1/1 only (launch_one / launch_b16_one); LZ for the forward
    classes 3/1, 3/2 and 1/1.

Entries the tuner left on the row kernel (32) stay there: it sums in another order by design and is chosen by eligibility.
Reference layers: model/backbone/dla.py:12-51,124-132,280-298, model/backbone/dla_neck.py:30-38,94-106,
model/dense_heads/monocon_heads.py:114-131 (forward, and under autograd for the gradients)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_err, GOLDEN_SEED
from hipmonocon import synth
from test_hip_ops import CONV_CASES, DGRAD_CASES, TOL, nhwc, rnd
from test_hip_train_step import build, check_step_vs_oracle, oracle_step_reference, to_cuda

pytestmark = pytest.mark.gpu

MODES = {0: "fp32", 1: "bf16", 2: "bf16x3", 3: "f16x2"}
TILINGS = (1, 4, 5, 6, 7, 8)                       # (2 and 3 are retired: no entry in CONV_SHAPES, refused as shape ids)
BNT = {1: 128, 4: 64, 5: 64, 6: 32, 7: 128, 8: 64}    # column tile of a shape: WN * WTN * 32 of conv_shape() (conv_mfma.h)
CFG_WS, CFG_SMALL, CFG_WRES = 16, 32, 64


def conv_coutp(cout):
    """padded column count of a layer (conv_ntile / conv_coutp, conv_mfma.h)"""
    t = 128 if cout >= 128 else (64 if cout > 32 else 32)
    return (cout + t - 1) // t * t


def patches(h, w):
    return ((w + 7) // 8) * ((h + 3) // 4)


# ------------------------------------------------------------------------------------------------ 1. op-level matrix
# A workgroup owns PB = 2 or 4 consecutive 4x8-pixel patches of ONE image: the patch count per image modulo 4 decides whether
# the last workgroup of image 0 is partly empty (and must not spill into image 1).
CONV_EXTRA = [
    # (name, B, H, W, [Cin...], Cout, k, stride, residual, relu, affine)
    ("s1_9x17_rem1", 2, 9, 17, [64], 64, 3, 1, True, True, True),               # 9 patches; W % 8 and H % 4 both non-zero
    ("s1_7x20_rem2", 2, 7, 20, [32], 128, 3, 1, False, True, True),             # 6 patches, 128 columns
    ("s1_3x50_rem3_c48", 2, 3, 50, [48], 64, 3, 1, True, False, True),          # 7 patches; 48 channels: the fp32 CK = 16 kernels
    ("s1_c16_to64", 1, 8, 24, [16], 64, 3, 1, False, True, True),               # CK = 16 at the 64-column shapes
    ("s2_odd_13x35", 2, 13, 35, [32], 64, 3, 2, False, True, True),             # odd input -> 7x18, 6 patches
    ("s2_64_128", 2, 12, 20, [64], 128, 3, 2, True, True, True),                # -> 6x10, 4 patches
    ("s2_c16_to64", 2, 10, 12, [16], 64, 3, 2, False, True, True),              # -> 5x6, 2 patches
    ("k1_c16_c48_to128", 2, 5, 12, [16, 48], 128, 1, 1, False, True, True),     # 1x1, CK = 16 at the 128-column shapes
    ("head_576_b2_rem2", 2, 7, 20, [64], 576, 3, 1, False, False, True),        # CoutP 640: the last 128-column tile is half padding
]
DGRAD_EXTRA = [
    # (name, B, Hin, Win, CinTotal, c_off, Cs, Cout, k, stride)
    ("dg_s1_9x17_rem1", 2, 9, 17, 64, 0, 64, 64, 3, 1),
    ("dg_s1_7x20_rem2", 2, 7, 20, 128, 0, 128, 32, 3, 1),
    ("dg_s1_3x50_rem3_dy48", 2, 3, 50, 64, 0, 64, 48, 3, 1),                    # dY of 48 channels: CK = 16, never the bf16 pipe
    ("dg_s1_dy16_2x4", 2, 2, 4, 64, 0, 64, 16, 3, 1),                           # smaller than one workgroup's pixels
    ("dg_s2_14x36_32_64", 2, 14, 36, 32, 0, 32, 64, 3, 2),                      # dY 7x18 (the nearest even size to 13x35)
    ("dg_s2_14x36_64_128", 2, 14, 36, 64, 0, 64, 128, 3, 2),                    # 6 patches per class at the 64-column shapes
    ("dg_s2_128_256", 2, 12, 20, 128, 0, 128, 256, 3, 2),                       # dY 6x10: 4 patches at the 128-column shapes
    ("dg_k1_slice_128", 2, 5, 12, 256, 128, 128, 64, 1, 1),
]
ALL_CONV = CONV_CASES + CONV_EXTRA
ALL_DGRAD = DGRAD_CASES + DGRAD_EXTRA


def test_the_case_lists_hold_the_edge_shapes():
    """the shapes section 1 promises are in the lists (a list edited later cannot lose one silently)"""
    def out_hw(c):
        k, s = c[6], c[7]
        return (c[2] + 2 * (k // 2) - k) // s + 1, (c[3] + 2 * (k // 2) - k) // s + 1
    fwd = {(patches(*out_hw(c)) % 4) for c in ALL_CONV if c[1] >= 2}
    dg = {(patches(-(-c[2] // c[9]), -(-c[3] // c[9])) % 4) for c in ALL_DGRAD if c[1] >= 2}
    assert {1, 2, 3} <= fwd and {1, 2, 3} <= dg
    assert any(out_hw(c)[0] % 4 and out_hw(c)[1] % 8 for c in ALL_CONV) and any(c[2] % 4 and c[3] % 8 for c in ALL_DGRAD if c[9] == 1)
    assert any(out_hw(c) == (2, 4) for c in ALL_CONV) and any((c[2], c[3]) == (2, 4) for c in ALL_DGRAD)
    assert any(c[7] == 2 and (c[2] % 2 or c[3] % 2) for c in ALL_CONV)
    for cin, cout in ((32, 64), (64, 128), (256, 512)):
        assert any(c[7] == 2 and c[4] == [cin] and c[5] == cout for c in ALL_CONV)
        assert any(c[9] == 2 and c[6] == cin and c[7] == cout for c in ALL_DGRAD)
    assert {3, 4} <= {len(c[4]) for c in ALL_CONV if c[6] == 1}
    assert sum(c[5] == 576 for c in ALL_CONV) >= 2 and any(c[7] == 576 for c in ALL_DGRAD)
    assert any(16 in c[4] for c in ALL_CONV) and any(48 in c[4] for c in ALL_CONV) and any(c[7] in (16, 48) for c in ALL_DGRAD)


def eligible_ids(mode, coutp, src_channels, ks, stride, hout, wout, dgrad):
    """shape ids a launch accepts (launch_conv, conv_mfma.hip): a tiling whose column tile divides the padded column count;
    its wave-specialised variant where the fp32 MFMA kernel runs (mode 0, or a source the bf16 pipe does not take) -- forward
    and stride-1 data gradients only, the parity classes of a stride-2 data gradient drop the flag; the weight-resident
    kernel in mode 3 where conv_wres_ok holds"""
    ids = [t for t in TILINGS if coutp % BNT[t] == 0]
    fp32_kernel = mode == 0 or any(c % 32 for c in src_channels)
    if fp32_kernel and not (dgrad and stride == 2):
        ids += [t | CFG_WS for t in TILINGS if coutp % BNT[t] == 0]
    if (mode == 3 and ks == 3 and stride == 1 and list(src_channels) == [64] and coutp % 64 == 0 and wout % 8 == 0
            and hout % 4 == 0):
        ids.append(4 | CFG_WRES)
    return ids


@pytest.fixture(scope="module")
def engines():
    from hipmonocon.engine import Engine
    es = {}
    for mode in MODES:
        es[mode] = Engine()
        es[mode].set_precision(mode)
    yield es
    for e in es.values():
        e.close()


_conv_ref = {}


def conv_reference(case):
    """inputs and the fp64 references of a forward case, computed once and shared by the four modes: exact, and with both
    operands rounded to bf16 first (what mode 1 is specified to compute)"""
    name, B, H, W, cins, cout, k, stride, use_res, relu, affine = case
    if name not in _conv_ref:
        seed = 2100 + ALL_CONV.index(case)
        xs = [rnd(seed, "x%d" % i, (B, c, H, W)) for i, c in enumerate(cins)]
        w = rnd(seed, "w", (cout, sum(cins), k, k), (2.0 / (k * k * sum(cins))) ** 0.5)
        scale = (1.0 + 0.1 * rnd(seed, "sc", (cout,))) if affine else None
        bias = 0.1 * rnd(seed, "bi", (cout,)) if affine else None
        Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
        res = rnd(seed, "res", (B, cout, Ho, Wo)) if use_res else None

        def ref(xcat, ww):
            r = F.conv2d(xcat, ww, None, stride, k // 2)
            if affine:
                r = r * scale.double()[None, :, None, None] + bias.double()[None, :, None, None]
            if use_res:
                r = r + res.double()
            return F.relu(r) if relu else r
        xcat = torch.cat(xs, 1)
        _conv_ref[name] = (xs, w, scale, bias, res, ref(xcat.double(), w.double()), ref(xcat.bfloat16().double(), w.bfloat16().double()))
    return _conv_ref[name]


@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
@pytest.mark.parametrize("case", ALL_CONV, ids=[c[0] for c in ALL_CONV])
def test_conv_every_shape_is_bit_identical(engines, case, mode):
    name, B, H, W, cins, cout, k, stride, use_res, relu, affine = case
    xs, w, scale, bias, res, exact, rounded = conv_reference(case)
    eng = engines[mode]
    dev = eng.device
    args = ([nhwc(x).to(dev) for x in xs], w.to(dev), stride, scale.to(dev) if affine else None, bias.to(dev) if affine else None,
            nhwc(res).to(dev) if use_res else None, relu)
    ids = eligible_ids(mode, conv_coutp(cout), cins, k, stride, exact.shape[2], exact.shape[3], False)
    try:
        base = eng.op_conv(*args)
        got = {}
        for cfg in ids:
            eng.set_conv_cfg(cfg)
            got[cfg] = eng.op_conv(*args)
    finally:
        eng.set_conv_cfg(0)
    for cfg in ids:
        assert torch.equal(got[cfg], base), (name, MODES[mode], cfg)
    out = base.cpu().permute(0, 3, 1, 2)
    assert out.shape == exact.shape
    bf16_pipe = mode >= 1 and all(c % 32 == 0 for c in cins)       # conv_bf16_ok; other sources stay on the fp32 MFMA kernel
    if mode == 1 and bf16_pipe:
        assert rel_err(out, rounded) < 2e-5          # fp32 accumulation of exactly-rounded operands (test_conv_bf16_operands)
    else:
        assert rel_err(out, exact) < (5e-6 if bf16_pipe else TOL)   # test_conv_split_emulation_is_fp32_accurate / test_conv


_dgrad_ref = {}


def dgrad_reference(case):
    name, B, H, W, cin_total, c_off, cs, cout, k, stride = case
    if name not in _dgrad_ref:
        seed = 2300 + ALL_DGRAD.index(case)
        Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
        w = rnd(seed, "w", (cout, cin_total, k, k), (2.0 / (k * k * cin_total)) ** 0.5)
        dy = rnd(seed, "dy", (B, cout, Ho, Wo))
        base = rnd(seed, "acc", (B, cs, H, W))

        def ref(ww, d):
            x = torch.zeros(B, cin_total, H, W, dtype=torch.float64, requires_grad=True)
            F.conv2d(x, ww, None, stride, k // 2).backward(d)
            return x.grad[:, c_off:c_off + cs].clone()
        _dgrad_ref[name] = (w, dy, base, ref(w.double(), dy.double()), ref(w.bfloat16().double(), dy.bfloat16().double()))
    return _dgrad_ref[name]


@pytest.mark.parametrize("mode", sorted(MODES), ids=[MODES[m] for m in sorted(MODES)])
@pytest.mark.parametrize("case", ALL_DGRAD, ids=[c[0] for c in ALL_DGRAD])
def test_conv_dgrad_every_shape_is_bit_identical(engines, case, mode):
    """the launches the train plan emits (flipped panel for stride 1, four output-parity classes scattering into dx for
    stride 2), plain and accumulating into an existing gradient"""
    name, B, H, W, cin_total, c_off, cs, cout, k, stride = case
    w, dy, acc0, exact, rounded = dgrad_reference(case)
    eng = engines[mode]
    dev = eng.device
    dyd, wd, accd = nhwc(dy).to(dev), w.to(dev), nhwc(acc0).to(dev)
    ids = eligible_ids(mode, conv_coutp(cs), [cout], k, stride, H, W, True)     # a conv over dY with Cs (padded) columns

    def run():
        out = eng.op_conv_dgrad(dyd, wd, (H, W), c_off, cs, stride)
        acc = accd.clone()
        eng.op_conv_dgrad(dyd, wd, (H, W), c_off, cs, stride, accumulate_into=acc)
        return out, acc
    try:
        base = run()
        got = {}
        for cfg in ids:
            eng.set_conv_cfg(cfg)
            got[cfg] = run()
    finally:
        eng.set_conv_cfg(0)
    for cfg in ids:
        assert torch.equal(got[cfg][0], base[0]), (name, MODES[mode], cfg)
        assert torch.equal(got[cfg][1], base[1]), (name, MODES[mode], cfg, "accumulate")
    out, acc = (t.cpu().permute(0, 3, 1, 2) for t in base)
    bf16_pipe = mode >= 1 and cout % 32 == 0          # mc_op_conv_dgrad packs the bf16 / fp16 panel for these only
    if mode == 1 and bf16_pipe:
        ref, tol = rounded, 2e-5
    elif bf16_pipe:
        ref, tol = exact, 5e-6                        # test_dgrad_on_the_bf16_pipe
    else:
        ref, tol = exact, (TOL if cout * k * k <= 4608 else 5e-6)        # test_conv_dgrad: one fp32 FMA chain over Cout*k*k terms
    assert rel_err(out, ref) < tol
    assert rel_err(acc, ref + acc0.double()) < tol


def test_stride2_dgrad_refuses_an_odd_input_size(engines):
    """13x35 -> 7x18 exists forward (s2_odd_13x35); its data gradient entry point takes even sizes only (the four parity
    classes are equally large) and says so instead of launching"""
    from hipmonocon.lib import MonoconHipError
    eng = engines[0]
    dy = torch.zeros(1, 7, 18, 64, device=eng.device)
    w = torch.zeros(64, 32, 3, 3, device=eng.device)
    with pytest.raises(MonoconHipError, match="even"):
        eng.op_conv_dgrad(dy, w, (13, 35), 0, 32, 2)


# ------------------------------------------------------------------------------------------------ 2. whole plans
def parse_table(table):
    """[key length, key..., id] per entry -> [(key, id)]; key = B, Hin, Win, ks, stride, Cout, CoutP, nsrc, flags, C_0..
    with flags = res | 2 * prec (bf16 pipe) | 64 (lazy source)  (mc_choose_conv_cfg)"""
    out, o = [], 0
    while o < len(table):
        kl = table[o]
        out.append((tuple(table[o + 1:o + 1 + kl]), table[o + 1 + kl]))
        o += kl + 2
    assert o == len(table)
    return out


def flat_table(entries):
    return [v for key, cfg in entries for v in (len(key), *key, cfg)]


def dictate(entries, T):
    """every entry takes shape T where its column tile divides the entry's padded column count, 128x32 (which divides every
    count) elsewhere; entries on the row kernel stay: it sums in a different order by design"""
    return [(key, cfg if cfg == CFG_SMALL else (T if key[6] % BNT[T & 15] == 0 else 6)) for key, cfg in entries]


PLAN_SHAPE = (2, 96, 160)
LAZY_ENV = {"MONOCON_HIP_LAZY_Z": "3", "MONOCON_HIP_LAZY_MIN": "0"}
PLAN_VARIANTS = {"fp32": ("fp32", {}), "bf16x3": ("bf16x3", {}), "f16x2": ("f16x2", {}), "f16x2-lazy": ("f16x2", LAZY_ENV)}
PLAN_RUNS = ([(v, T) for v in PLAN_VARIANTS for T in (1, 4, 5, 7, 8)] + [("fp32", T | CFG_WS) for T in (1, 5, 7, 8)]
             + [("f16x2", 4 | CFG_WRES), ("f16x2-lazy", 4 | CFG_WRES)])
PLAN_ENV_KEYS = ("MONOCON_HIP_LAZY_Z", "MONOCON_HIP_LAZY_MIN", "MONOCON_HIP_ZBITS", "MONOCON_HIP_LAZY_FEAT", "MONOCON_HIP_BM_EPILOGUE",
                 "MONOCON_HIP_WRES_BWD", "MONOCON_HIP_DGRAD_S2_THIN", "MONOCON_HIP_TUNE_CACHE", "MONOCON_HIP_AUTOTUNE")
_plan = {}         # variant -> (entries exported by an autotuned plan build, the 128x32 run)
_batch = {}


def plan_batch():
    if not _batch:
        _batch["cpu"] = synth.make_batch(GOLDEN_SEED + 9, *PLAN_SHAPE)
        _batch["gpu"] = to_cuda(_batch["cpu"])
    return _batch


def set_plan_env(monkeypatch, variant):
    for k in PLAN_ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in PLAN_VARIANTS[variant][1].items():
        monkeypatch.setenv(k, v)                  # read when the train plan is built
    monkeypatch.setenv("MONOCON_HIP_PLAN_DEBUG", "1")


def bound_engine(m):
    from hipmonocon.train import _binding
    return m._rt.get(_binding(m).state(m))       # the handle forward_train will use, parameters and gradient buffers bound


def dictated_step(sd, variant, entries, capfd):
    """one forward + backward on a fresh model whose every conv shape comes from `entries`; returns losses, all parameter
    gradients, all buffers, and the shape ids on the plan's backward-statistics twin lines"""
    table = flat_table(entries)
    m = build(sd, PLAN_VARIANTS[variant][0])
    eng = bound_engine(m)
    assert eng.tune_export() == []
    assert eng.tune_import(table) == len(entries)
    capfd.readouterr()
    _, loss = m(plan_batch()["gpu"])
    sum(loss.values()).backward()
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    # a grown table means some launch was tuned instead of dictated: such a run proves nothing
    assert eng.tune_export() == table
    twins = [int(l.split(" cfg ")[1].split()[0]) for l in err.splitlines() if l.startswith("[plan]   twin of")]
    return {"m": m, "loss": loss,
            "losses": torch.stack([v.detach() for v in loss.values()]).clone(),
            "grads": torch.cat([p.grad.flatten() for p in m.parameters() if p.grad is not None]).clone(),
            "buffers": torch.cat([b.flatten().float() for b in m.buffers()]).clone(), "twins": twins}


def plan_base(sd, variant, monkeypatch, capfd):
    if variant not in _plan:
        set_plan_env(monkeypatch, variant)
        m = build(sd, PLAN_VARIANTS[variant][0])
        eng = bound_engine(m)
        eng.build_train_plan(*PLAN_SHAPE)
        entries = parse_table(eng.tune_export())
        del m, eng
        _plan[variant] = (entries, dictated_step(sd, variant, dictate(entries, 6), capfd))
    return _plan[variant]


@pytest.mark.parametrize("variant", list(PLAN_VARIANTS))
def test_plan_on_the_128x32_tiling_meets_the_oracle(golden_sd, variant, monkeypatch, capfd):
    """the run every other tiling is compared with: losses within 1e-4 of the oracle in fp64, gradient norm of the oracle's
    (the check of test_train_forward_shape_sweep_vs_oracle)"""
    set_plan_env(monkeypatch, variant)
    entries, base = plan_base(golden_sd, variant, monkeypatch, capfd)
    if "oracle" not in _batch:
        _batch["oracle"] = oracle_step_reference(golden_sd, plan_batch()["cpu"])
    check_step_vs_oracle(base["m"], base["loss"], *_batch["oracle"])
    assert 6 in base["twins"]
    lazy_keys = [key for key, _ in entries if key[8] & 64]
    if variant == "f16x2-lazy":
        assert len(lazy_keys) >= 10, len(lazy_keys)       # the LZ instantiations are reached
    if not variant.startswith("f16x2"):
        assert not lazy_keys


@pytest.mark.parametrize("variant,T", PLAN_RUNS, ids=["%s-%d" % r for r in PLAN_RUNS])
def test_train_step_is_bit_identical_on_every_tiling(golden_sd, variant, T, monkeypatch, capfd):
    set_plan_env(monkeypatch, variant)
    entries, base = plan_base(golden_sd, variant, monkeypatch, capfd)
    dictated = dictate(entries, T)
    assert any(cfg == T for _, cfg in dictated)
    run = dictated_step(golden_sd, variant, dictated, capfd)
    # the backward-statistics (BM) launches print their shape id: T reached at least one of them (the flags of a variant do not
    # apply to a twin -- the wave-specialised kernel has no such epilogue, backward launches drop the weight-resident flag)
    assert any(t & 15 == T & 15 for t in run["twins"]), run["twins"]
    assert torch.equal(run["losses"], base["losses"])
    assert torch.equal(run["grads"], base["grads"])
    assert torch.equal(run["buffers"], base["buffers"])
    assert bool(torch.isfinite(run["grads"]).all())


@pytest.mark.parametrize("variant", list(PLAN_VARIANTS))
def test_plan_matrix_covers_every_conv_class(golden_sd, variant, monkeypatch, capfd):
    """from the exported table: every (ks, stride) class the tuner decides is present, every tiling is written into each class
    that has a divisible column count, and no class is left with fewer than two distinct tilings"""
    set_plan_env(monkeypatch, variant)
    entries, _ = plan_base(golden_sd, variant, monkeypatch, capfd)
    # the row kernel is taken by eligibility before the table is consulted: an entry naming it could only come from timing it
    # against the tilings, whose sums it does not reproduce -- no signature of this network is decided that way
    assert not [key for key, cfg in entries if cfg == CFG_SMALL]
    tiled = [(key, cfg) for key, cfg in entries if cfg != CFG_SMALL]
    classes = sorted({(key[3], key[4]) for key, _ in tiled})
    assert classes == [(1, 1), (3, 1), (3, 2), (12, 1), (21, 1), (22, 1)], classes
    for cls in classes:
        reached = set()
        for T in TILINGS:
            hit = {cfg for key, cfg in dictate(tiled, T) if (key[3], key[4]) == cls}
            if any(key[6] % BNT[T] == 0 for key, _ in tiled if (key[3], key[4]) == cls):
                assert T in hit, (cls, T)
            reached |= hit
        print("%s %s: tilings %s" % (variant, cls, sorted(reached)))
        assert len(reached) >= 2, (cls, reached)
    prec_flag = {"fp32": 0, "bf16x3": 4, "f16x2": 6}[PLAN_VARIANTS[variant][0]]
    assert {key[8] & 6 for key, _ in tiled} <= {0, prec_flag}
    if prec_flag:
        assert sum((key[8] & 6) == prec_flag for key, _ in tiled) >= len(tiled) // 2       # the bf16 / fp16 pipe kernels carry the plan


# ---- eval forward
EVAL_MODES = {"fp32": 0, "bf16x3": 2, "f16x2": 3}
_eval = {}


def eval_forward(sd, mode, img, table):
    from hipmonocon.engine import Engine
    e = Engine()
    try:
        e.set_precision(mode)
        e.bind_state(sd)
        if table is not None:
            assert e.tune_import(table) >= 1
        preds = {k: v.clone() for k, v in e.forward_infer(img).items()}
        torch.cuda.synchronize()
        return preds, e.tune_export()
    finally:
        e.close()


def eval_base(golden_sd, precision, monkeypatch):
    monkeypatch.delenv("MONOCON_HIP_TUNE_CACHE", raising=False)
    monkeypatch.delenv("MONOCON_HIP_AUTOTUNE", raising=False)
    if precision not in _eval:
        sd = {k: v.cuda() for k, v in golden_sd.items()}
        img = synth.make_batch(GOLDEN_SEED + 1, 2, 64, 128, with_labels=False)["img"].cuda()
        _, tuned = eval_forward(sd, EVAL_MODES[precision], img, None)       # autotuning on: the eval plan's keys
        entries = parse_table(tuned)
        table = flat_table(dictate(entries, 6))
        preds, after = eval_forward(sd, EVAL_MODES[precision], img, table)
        assert after == table
        _eval[precision] = (sd, img, entries, preds)
    return _eval[precision]


@pytest.mark.parametrize("precision", list(EVAL_MODES))
@pytest.mark.parametrize("T", TILINGS)
def test_eval_forward_is_bit_identical_on_every_tiling(golden_sd, precision, T, monkeypatch):
    """mc_forward_infer with every conv shape dictated: all ten prediction maps bit-identical to the 128x32 run, which meets
    the reference's fp64 golden at the gate of test_small_eval_forward_vs_reference_golden"""
    sd, img, entries, base = eval_base(golden_sd, precision, monkeypatch)
    assert len(base) == 10
    if T == 6:
        g = load_golden("fwd_small_eval.npz")
        for k, v in base.items():
            assert rel_err(v.cpu(), g["f64." + k]) < 1e-4, k
        assert {(key[3], key[4]) for key, cfg in entries if cfg != CFG_SMALL} == {(3, 1), (3, 2), (1, 1)}
        return
    dictated = dictate(entries, T)
    assert any(cfg == T for _, cfg in dictated)
    table = flat_table(dictated)
    preds, after = eval_forward(sd, EVAL_MODES[precision], img, table)
    assert after == table
    for k in base:
        assert torch.equal(preds[k], base[k]), (k, T)


# ------------------------------------------------------------------------------------------------ 3. obeyed or refused
def test_a_table_naming_an_indivisible_tiling_is_refused_whole(golden_sd, monkeypatch, capfd):
    """128x128 (id 1) for a signature of 64 padded columns: mc_tune_import checks every entry's column tile against its key
    on the host and adopts NOTHING of such a table -- no plan is built from it and nothing runs on the device; the same
    process then builds and runs a plan from a valid table on a fresh handle"""
    from hipmonocon.lib import MonoconHipError
    set_plan_env(monkeypatch, "fp32")
    entries, base = plan_base(golden_sd, "fp32", monkeypatch, capfd)
    victim = max(i for i, (key, cfg) in enumerate(entries) if key[6] == 64 and cfg != CFG_SMALL)
    bad = dictate(entries, 6)
    bad[victim] = (bad[victim][0], 1)
    m = build(golden_sd, "fp32")
    eng = bound_engine(m)
    with pytest.raises(MonoconHipError, match="does not divide"):
        eng.tune_import(flat_table(bad))
        eng.build_train_plan(*PLAN_SHAPE)
    assert eng.tune_export() == []                # not half-applied: the entries in front of the bad one are not adopted either
    del m, eng
    run = dictated_step(golden_sd, "fp32", dictate(entries, 6), capfd)
    assert torch.equal(run["losses"], base["losses"]) and torch.equal(run["grads"], base["grads"])


def test_the_retired_ids_are_no_shape_ids():
    """ids 2 and 3 (256x64, 256x32) have no entry in CONV_SHAPES (conv_mfma.h): mc_set_conv_cfg and mc_tune_import refuse them
    as they refuse any unknown id, on the host and before anything is built -- not at the first launch of a plan"""
    from hipmonocon.engine import Engine
    from hipmonocon.lib import MonoconHipError
    eng = Engine(0)
    key = (2, 96, 160, 3, 1, 64, 64, 1, 0, 64)        # B, Hin, Win, ks, stride, Cout, CoutP, nsrc, flags, C_0
    for cfg in (2, 3, 2 | CFG_WS):
        with pytest.raises(MonoconHipError, match="unknown shape id"):
            eng.set_conv_cfg(cfg)
    with pytest.raises(MonoconHipError, match="unknown shape id"):
        eng.tune_import(flat_table([(key, 2)]))
    assert eng.tune_export() == []
    eng.set_conv_cfg(6)
    assert eng.tune_import(flat_table([(key, 6)])) == 1
    assert parse_table(eng.tune_export()) == [(key, 6)]
    eng.close()
