"""The train-mode dense heads against fp64 at fp32 round-off, at the batch sizes training uses (B = 2 ... 64).

`MonoConDenseHeads.forward_train(feat, data)` (mc_head_forward_train, mc_head_backward_pred_grads; csrc/kernels_head_train.hip:
attn_train_fwd_kernel, inst_stats_kernel, head_bwd_kernel in its three modes, head_dx, attn_train_bwd_kernel,
dpred_pack_kernel<USER>) on a given float32 `feat`, against the oracle's own head code (`O.head_predictions`, autograd) on the host
from the same float32 inputs: in float64 -- the truth -- and in float32 -- the yard-stick.

The objective is the pure map term J = sum_k <G_k, pred_k> / (C_k h w), G_k ~ N(0, 1) from a seeded CPU generator; no loss
enters it.  The backward is then ONE linear chain (USER pack with the derivatives of the clamped sigmoid and of the depth
transform, the nine 1x1 weight and data gradients, the ReLU mask, the AttnBN backward with its attention branch through BN(10)
over the batch and the hard sigmoid, the fused 576-channel 3x3 weight, bias and data gradient), and the only places where a
float32 and a float64 run may take different branches are dealt with one by one:

  hidden ReLU       G is zero at the pixels of a head where any of its 64 post-AttnBN values lies within 1e-4 channel standard
                    deviations of zero in fp64 (plan_graph.head_decided_pixels, shared with test_hip_pred_grads.py); at most 2 %
                    of a head's B h w pixels
  heat-map clamp    G is zero at the elements whose fp64 sigmoid lies within 1e-6 of 1e-4 or 1 - 1e-4
  hard sigmoid      relu6(t + 3) / 6 is decided once per (image, head, attention component) and cannot be masked: the feat seed
                    of every (case, state) was chosen on the CPU so that no fp64 t lies within 1e-4 of -3 or +3; asserted, and
                    the float32 yard-stick's t must agree with the fp64 one to a tenth of that margin

Gate per tensor kind and case: 5 x the worst float32-yard-stick error of the kind in the case + 4 x 2^-24, on the relative L2
error ||got - ref64|| / ||ref64|| (the 5 of test_gradients_match_reference / test_hip_backward_layers.py).  f16x2 and bf16x3 get
the same gate.  Every partition claim of a case is derived from the launcher's own formula and asserted.  "A tenth of that
margin" is a tenth of the CASE's margin, which is asserted to be at least 1e-4: the float32 oracle's own t is 1e-5 .. 9e-5 from the
fp64 one (3e-5 .. 2e-4 at B = 2, where BN(10) sees two samples; 4e-5 .. 6e-5 at B = 64), so no seed meets a tenth of 1e-4 itself.

In f16x2 the 3x3 weight gradients alone get one more term, the operand floor of the format (`f16x2_floor`): the nine heads' dx is
ONE operand tensor with ONE exponent, and an element more than 2^-17 below its maximum is stored with an absolute error of up
to 2^-39 of that maximum.  On the plain and attention-stressed states the term is 1e-9 .. 5e-8 of a gradient's norm -- nothing;
on the output-stressed state the depth head's dx (steep end of its transform: max |dx| 2e6) lies eleven decades above the
others', and seven heads' 3x3 weight gradients come out 5e-3 .. 4e-1 wrong in f16x2 (1e-5 in fp32), 1/100 .. 1/36 of what the
floor allows.  No other kind and no other mode needs a term.

MEASURED on an MI355X: worst HIP error / float32 yard-stick error per kind (a gate is reached at 5 + 4 x 2^-24 / yard-stick)
run                           3x3 W    3x3 b    1x1 W    1x1 b  att.0 W  attBN W  attBN b  weight_    bias_     feat     maps  buffers
b2/plain fp32                  0.92     0.21     1.15     0.25     0.25     0.91     1.80     1.03     1.01     1.23     1.79     0.76
b2/plain f16x2                 1.01     1.00     0.60     0.12     1.00     0.98     0.72     0.56     0.57     0.85     1.42     0.82
b9/plain fp32                  0.40     0.31     1.36     0.48     0.31     0.84     3.00     1.17     0.97     2.65     1.88     0.77
b9/plain f16x2                 0.31     0.14     0.83     0.48     0.19     1.03     0.82     1.02     0.91     1.28     1.05     0.98
b17/plain fp32                 0.52     0.48     1.46     0.37     0.97     1.46     2.91     1.15     0.83     3.59     1.68     1.16
b17/plain f16x2                0.45     0.38     0.70     0.41     0.74     0.89     0.78     0.86     0.78     1.46     0.86     1.16
b32/plain fp32                 0.50     0.45     1.36     0.14     0.74     1.23     1.90     1.37     0.91     3.74     1.78     1.20
b32/plain f16x2                0.57     0.62     0.78     0.14     0.84     1.59     0.66     1.00     0.87     1.47     0.86     1.50
b32/plain bf16x3               0.49     0.47     0.69     0.12     0.71     0.78     0.39     0.94     0.91     1.44     0.76     1.16
b32/attn fp32                  0.52     0.46     1.29     0.25     0.91     0.89     1.26     0.90     0.74     2.37     1.40     0.89
b32/attn f16x2 DX_FUSE=0       0.45     0.37     1.10     0.40     0.77     0.67     0.61     0.99     1.04     1.17     0.78     0.97
b32/attn f16x2 DX_FUSE=1       0.45     0.38     1.10     0.40     0.77     0.67     0.61     0.99     1.04     1.17     0.78     0.97
b32/out fp32                   2.42     0.26     1.88     2.41     1.30     2.03     3.11     1.84     2.08     5.04     2.62     1.20
b32/out f16x2              (floor)     0.23     0.79     1.03     0.79     0.92     0.98     0.94     1.00     1.44     1.00     1.50
b64/plain fp32                 0.61     0.26     0.96     0.11     1.10     1.46     1.82     1.03     1.01     1.89     1.34     1.00
b64/plain f16x2 DX_FUSE=0      0.73     0.24     0.77     0.05     1.03     1.00     0.49     0.98     0.95     1.11     0.90     0.94
b64/plain f16x2 DX_FUSE=1      0.73     0.25     0.77     0.05     1.03     1.00     0.49     0.98     0.95     1.11     0.90     0.94
the float32 yard-stick itself (worst of the kind, on the GPU machine's host)
b2/plain                    2.9e-04  1.9e-02  3.7e-06  1.7e-06  1.1e-02  6.3e-05  2.1e-06  1.1e-05  1.0e-05  6.3e-06  6.4e-07  4.1e-07
b9/plain                    7.4e-06  1.5e-04  6.8e-07  7.7e-07  9.4e-05  5.5e-06  4.6e-06  1.5e-06  1.4e-06  4.9e-07  5.2e-07  2.4e-07
b17/plain                   1.2e-06  1.8e-05  5.9e-07  7.0e-07  6.0e-06  5.0e-06  8.4e-07  9.8e-07  9.5e-07  3.4e-07  4.8e-07  2.3e-07
b32/plain                   1.3e-06  1.6e-05  6.9e-07  1.3e-06  6.0e-06  3.0e-06  2.8e-06  1.0e-06  1.0e-06  3.3e-07  4.6e-07  1.6e-07
b32/attn                    2.4e-06  1.2e-05  1.0e-06  1.3e-06  2.9e-06  9.4e-06  1.3e-06  2.3e-06  2.7e-06  5.7e-07  6.9e-07  1.8e-07
b32/out                     4.3e-06  7.0e-05  5.2e-06  5.3e-06  7.4e-06  5.2e-06  3.6e-06  5.3e-06  5.4e-06  2.0e-06  2.9e-06  1.6e-07
b64/plain                   1.1e-05  4.3e-04  1.3e-06  3.8e-06  6.4e-05  9.5e-06  2.3e-06  3.3e-06  4.1e-06  7.4e-07  8.4e-07  7.9e-08
Closest to its gate: the feat gradient of b32/out in fp32, 1.03e-5 against 1.04e-5 (the fp32 data gradient of the fused 576-channel
conv, one accumulator over K = 5184 with the depth head's dx eleven decades above the rest; f16x2 has 2.9e-6 there).  At B = 2
BN(10) over two samples leaves t = +-gamma + beta almost whatever its input: the attention branch's gradients nearly cancel, and
the float32 oracle itself has 1e-2 on attention.0.weight and the 3x3 biases.  The loss objective at B = 32: feat 7.9e-7,
parameters 1.3e-5 at the worst (dim_head.0.bias), median 4.2e-7.
END MEASURED

GPU-only."""
import collections
import time

import numpy as np
import pytest
import torch

from hipmonocon import netspec, synth
from plan_graph import HEADS, HEAT_KEYS, head_attention_stress, head_decided_pixels, head_output_stress
from test_hip_head_zskip import TILE, partition, red_rows

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
KINK_MARGIN = 1e-4           # no fp64 hard-sigmoid input within this of -3 or +3
RELU_TAU = 1e-4              # hidden ReLU decisions closer than this (in channel standard deviations) are left out
CLAMP_TAU = 1e-6             # heat-map elements whose fp64 sigmoid is closer than this to a clamp are left out
LEFT_OUT_MAX = 0.02
LABEL_SEED = 812
G_SEED = 40

# name: (B, pad H, pad W)
SHAPES = {"b2": (2, 96, 320), "b9": (9, 64, 128), "b17": (17, 32, 64), "b32": (32, 32, 64), "b64": (64, 32, 992)}
# (case, state) -> feat seed, chosen on the CPU by the hard-sigmoid rule above (the first seed from 5 upwards that keeps every
# fp64 t at least KINK_MARGIN away from both kinks and the float32 yard-stick's t within a tenth of the case's margin)
FEAT_SEED = {("b2", "plain"): 5, ("b9", "plain"): 5, ("b17", "plain"): 5, ("b32", "plain"): 5, ("b32", "attn"): 6,
             ("b32", "out"): 5, ("b64", "plain"): 6}

KINDS = ("3x3 weights", "3x3 biases", "1x1 weights", "1x1 biases", "attention.0.weight", "attention BN weight",
         "attention BN bias", "weight_", "bias_", "feat", "prediction maps", "running buffers")


def kind_of(name):
    """the tensor kind of a head parameter (state_dict key without the `head.` prefix)"""
    if name.startswith("dir_cls.") or name.startswith("dir_reg.") or ".3." in name:
        return "1x1 weights" if name.endswith(".weight") else "1x1 biases"
    if name.endswith(".attention.0.weight"):
        return "attention.0.weight"
    if name.endswith(".attention.1.weight"):
        return "attention BN weight"
    if name.endswith(".attention.1.bias"):
        return "attention BN bias"
    if name.endswith(".weight_"):
        return "weight_"
    if name.endswith(".bias_"):
        return "bias_"
    assert name.endswith(".0.weight") or name.endswith(".0.bias"), name
    return "3x3 weights" if name.endswith(".weight") else "3x3 biases"


def rel_l2(got, ref):
    ref = ref.detach().double()
    return float((got.detach().cpu().double() - ref).norm() / max(float(ref.norm()), 1e-300))


# ------------------------------------------------------------------------------------------------ the launchers' partitions
def conv_patches(H, W):
    """partials per image of the fused head conv: one per 4x8 patch of the feature map (conv_chunks_per_image, conv_mfma.h)"""
    return ((W // 4 + 7) // 8) * ((H // 4 + 3) // 4)


def stats_main_parts(chunks):
    """how many of inst_stats_kernel's 16 parts enter its four-loads-in-flight main loop (`k + 48 < chunks`, k = part)"""
    return sum(1 for part in range(16) if part + 48 < chunks)


def prefetch_groups(B):
    """(groups of eight images the AttnBN kernels fetch, images in the last group): the tail's other slots are clamped to B - 1"""
    return (B + 7) // 8, B - 8 * ((B - 1) // 8)


def assert_partition(case):
    """what the case is in the suite for, from the launchers' own formulas: a retuned launcher fails here"""
    B, H, W = SHAPES[case]
    HW, bpi, rpb = partition(B, H, W)
    if case == "b2":
        assert (HW, bpi, rpb) == (1920, 60, 32) and conv_patches(H, W) == 60
        assert stats_main_parts(60) == 12                       # parts 0..11: main loop, 12..15: the tail alone
        assert stats_main_parts(bpi) == 12                      # (the backward sums its 60 row-block partials the same way)
    elif case == "b9":
        assert (HW, rpb) == (512, 32) and prefetch_groups(B) == (2, 1)
    elif case == "b17":
        assert (HW, rpb) == (128, 32) and prefetch_groups(B) == (3, 1) and conv_patches(H, W) == 4
        assert B > 16                                           # image 16 is row group 0's second turn (b = grp; b += 16)
    elif case == "b32":
        assert (HW, bpi, rpb) == (128, 4, 32) and prefetch_groups(B) == (4, 8)
    else:
        assert case == "b64" and B == 64                        # the ABI maximum
        assert red_rows(B, HW) == 128 and (HW, bpi, rpb) == (1984, 16, 124) and conv_patches(H, W) == 62
        assert rpb > TILE and rpb % TILE != 0                   # two staged blocks (64 + 60) that start off the tile grid
        assert stats_main_parts(62) == 14
        # the smallest HW at B = 64 whose workgroups straddle tiles: red_rows stays at 64 or below (divisors of the tile) until
        # 64 * ceil(HW / 128) >= 1024, i.e. HW >= 1921
        assert red_rows(B, 1920) == 64 and red_rows(B, 1921) == 128


# ------------------------------------------------------------------------------------------------ the two host references
def state_of(cond_sd, state):
    if state == "attn":
        return head_attention_stress(cond_sd)
    if state == "out":
        # cond_sd's head output weights are HEAD_OUT_SCALE (0.02) of the golden state's, for which head_output_stress's default
        # gains (12, 3) were chosen: the same logit ranges need the gains divided by that scale
        return head_output_stress(cond_sd, 12.0 / synth.HEAD_OUT_SCALE, 3.0 / synth.HEAD_OUT_SCALE)
    assert state == "plain"
    return cond_sd


def make_feat(seed, B, H, W):
    return torch.from_numpy(synth.normalish(seed, "feat", (B, 64, H // 4, W // 4)).astype(np.float32)).abs()


def oracle_run(sd, feat, dtype, Gs=None):
    """the oracle's train-mode head on `feat` in `dtype`: the ten maps, the hidden maps, the raw heat-map logits, the hard
    sigmoid's inputs t {head: (B, 10)}, the updated buffers, and -- with Gs {key: float32 map gradient} -- the gradients of
    J = sum_k <Gs_k, pred_k> with respect to feat and every head parameter"""
    from oracle import monocon_oracle as O

    class Ctx(O._Ctx):
        def __init__(self, sd_):
            super().__init__(sd_, True)
            self.hidden, self.raw, self.t, self.hidden_live = {}, {}, {}, {}

        def conv(self, x, name, stride=1, pad=0):
            y = super().conv(x, name, stride, pad)
            if name.endswith(".0") and pad == 1:
                self.hidden[name[len("head."):-2]] = y.detach()
                if y.requires_grad:
                    y.retain_grad()
                    self.hidden_live[name[len("head."):-2]] = y
            elif name in ("head.heatmap_head.3", "head.kpt_heatmap_head.3"):
                self.raw[O.HEAD_BRANCHES[name[len("head."):-2]]] = y.detach()
            return y

        def bn(self, x, name, *args, **kw):
            y = super().bn(x, name, *args, **kw)
            if name.endswith(".attn_weights.attention.1"):
                self.t[name[len("head."):-len(".1.attn_weights.attention.1")]] = y.detach().flatten(1)
            return y

    live = {k: (v.to(dtype).clone() if v.is_floating_point() else v.clone()) for k, v in sd.items() if k.startswith("head.")}
    params = [k for k, v in live.items() if v.is_floating_point() and "running" not in k]
    grad = Gs is not None
    for k in params:
        live[k].requires_grad_(grad)
    f = feat.to(dtype).clone().requires_grad_(grad)
    cx = Ctx(live)
    with torch.set_grad_enabled(grad):
        preds = O.head_predictions(cx, f)
        if grad:
            sum((Gs[k].to(dtype) * preds[k]).sum() for k in preds).backward()
    # dx, the gradient wrt the hidden maps (the operand of the fused 3x3 weight and data gradients): only its maximum over all
    # nine heads and its magnitude sum per channel are kept
    dx_max = max(float(y.grad.abs().max()) for y in cx.hidden_live.values()) if grad else None
    dx_sum = {br: y.grad.abs().sum((0, 2, 3)) for br, y in cx.hidden_live.items()} if grad else None
    R = collections.namedtuple("OracleRun", "preds hidden raw t buffers grads gfeat live dx_max dx_sum")
    return R({k: v.detach() for k, v in preds.items()}, cx.hidden, cx.raw, cx.t, cx.new_buffers,
             {k[len("head."):]: live[k].grad for k in params} if grad else None, f.grad if grad else None,
             {k: v.detach() for k, v in live.items()}, dx_max, dx_sum)


def f16x2_floor(R):
    """{3x3 weight name: norm of the f16x2 operand floor of its gradient}.  f16x2 splits an operand tensor into two fp16 pieces
    of x * 2^e with ONE exponent per tensor, max |x| 2^e in [2^14, 2^15).  An element keeps 22 bits of its own
    size until its pieces reach fp16's subnormals, whose spacing is 2^-24: from there the error is absolute, at most
    2^-25 / 2^e <= 2^-39 max |x| per element.  The nine heads' dx is ONE tensor: a head whose dx lies 2^-17 or more below the
    largest head's is stored with that absolute error, whatever its own size.  For dW[o][c][tap] = sum_p dx[o][p] feat[c][p + tap]
    the floors of both operands add up to at most 2^-39 (max |dx| sum_p |feat[c][p + tap]| + max |feat| sum_p |dx[o][p]|).  The
    22-bit part is not added: it is of the size of fp32's own rounding, which the 5 x yard-stick gate covers (every f16x2 case
    passes the plain gate unless the floor is reached)."""
    feat = R.feat.double().abs()
    B, C, h, w = feat.shape
    P = torch.nn.functional.pad(feat, (1, 1, 1, 1))
    S = torch.stack([torch.stack([P[:, :, r:r + h, s:s + w].sum((0, 2, 3)) for s in range(3)], -1) for r in range(3)], -2)  # (C, 3, 3)
    out = {}
    for br in HEADS:
        E = 2.0 ** -39 * (R.r64.dx_max * S[None] + float(feat.max()) * R.r64.dx_sum[br][:, None, None, None])
        out["%s.0.weight" % br] = float(E.norm())
    return out


def regimes(t):
    """(low, linear, high) counts of the hard sigmoid's inputs of one head"""
    return int((t <= -3).sum()), int(((t > -3) & (t < 3)).sum()), int((t >= 3).sum())


class Reference:
    """both host references of one (case, state), built once: G, the fp64 truth, the float32 yard-stick and the per-kind gates"""

    def __init__(self, cond_sd, case, state):
        t0 = time.time()
        B, H, W = SHAPES[case]
        self.case, self.state, self.shape = case, state, (B, H, W)
        self.sd = state_of(cond_sd, state)
        self.feat = make_feat(FEAT_SEED[(case, state)], B, H, W)
        h, w = H // 4, W // 4
        fwd = oracle_run(self.sd, self.feat, torch.float64)
        # ---- decisions
        keep = head_decided_pixels(fwd.live, fwd.hidden, RELU_TAU)
        self.left_out = {br: 1.0 - float(keep[br].double().mean()) for br in keep}
        self.regimes = {br: regimes(fwd.t[br]) for br in HEADS}
        self.kink = min(float((fwd.t[br].abs() - 3.0).abs().min()) for br in HEADS)
        gen = torch.Generator().manual_seed(G_SEED)
        self.Gs, self.clamp_left_out = {}, {}
        head_of = {v: k for k, v in _branches().items()}
        for k, c in netspec.PRED_KEYS:
            G = torch.randn((B, c, h, w), generator=gen, dtype=torch.float32)
            G = G * keep["dir_feat" if k.startswith("alpha_") else head_of[k]][:, None].float()
            if k in HEAT_KEYS:
                s = torch.sigmoid(fwd.raw[k])
                near = ((s - 1e-4).abs() <= CLAMP_TAU) | ((s - (1.0 - 1e-4)).abs() <= CLAMP_TAU)
                self.clamp_left_out[k] = int(near.sum())
                G = G * (~near).float()
            self.Gs[k] = (G.double() / (c * h * w)).float()          # J = sum_k <G_k, pred_k> / (C_k h w), the scale folded in
        self.r64 = oracle_run(self.sd, self.feat, torch.float64, self.Gs)
        self.r32 = oracle_run(self.sd, self.feat, torch.float32, self.Gs)
        self.t_diff = max(float((self.r32.t[br].double() - self.r64.t[br]).abs().max()) for br in HEADS)
        # ---- the yard-stick: the float32 oracle's error per tensor, worst per kind -> gate
        self.yard = collections.defaultdict(float)
        for kind, name, got, ref in self.pairs(self.r32.preds, self.r32.buffers, self.r32.gfeat, self.r32.grads):
            self.yard[kind] = max(self.yard[kind], rel_l2(got, ref))
        self.gate = {k: 5.0 * self.yard[k] + 4.0 * U24 for k in KINDS}
        self.seconds = time.time() - t0

    def pairs(self, preds, buffers, gfeat, grads):
        """(kind, name, value, fp64 reference) of everything compared; buffers: `head.`-prefixed keys, grads: without"""
        for k in self.r64.preds:
            yield "prediction maps", k, preds[k], self.r64.preds[k]
        for k, v in self.r64.buffers.items():
            if not k.endswith("num_batches_tracked"):
                yield "running buffers", k, buffers[k], v
        yield "feat", "feat", gfeat, self.r64.gfeat
        for n, ref in self.r64.grads.items():
            if ref is not None:
                yield kind_of(n), n, grads[n], ref

    def check_conditions(self):
        """what the case rests on: its left-out share, its regime counts, its kink margin"""
        B = self.shape[0]
        assert set(self.left_out) == set(HEADS)
        assert max(self.left_out.values()) <= LEFT_OUT_MAX, self.left_out
        for k, n in self.clamp_left_out.items():
            assert n <= LEFT_OUT_MAX * self.r64.preds[k].numel(), (k, n)
        assert self.kink >= KINK_MARGIN, self.kink
        assert self.t_diff < 0.1 * self.kink, (self.t_diff, self.kink)
        for br in HEADS:
            lo, lin, hi = self.regimes[br]
            assert lo + lin + hi == 10 * B
            assert regimes(self.r32.t[br]) == (lo, lin, hi), br          # the yard-stick took the same branches
            if self.state == "attn":
                assert lo > 0 and lin > 0 and hi > 0, (br, lo, lin, hi)
        if self.state == "out":
            # both clamps and the interior of a heat map carry values, and the depth logit reaches its steep end
            for k in HEAT_KEYS:
                s = torch.sigmoid(self.r64.raw[k])
                assert bool((s < 1e-4).any()) and bool((s > 1 - 1e-4).any()) and bool(((s > 0.01) & (s < 0.99)).any()), k
            assert float(self.r64.preds["depth_pred"][:, 0].max()) > 1e3


def _branches():
    from oracle import monocon_oracle as O
    return O.HEAD_BRANCHES


_REFS = {}


def reference(cond_sd, case, state):
    """module-scoped cache: one reference pair per (case, state), shared by all its precisions and switches, never changed"""
    if (case, state) not in _REFS:
        _REFS[(case, state)] = Reference(cond_sd, case, state)
        R = _REFS[(case, state)]
        print("%s/%s: host references in %.1f s; left out <= %.2f %% of a head's pixels, clamp %s; kink margin %.2e, "
              "|t32 - t64| <= %.1e; regimes (low, linear, high) %s"
              % (case, state, R.seconds, 100 * max(R.left_out.values()), R.clamp_left_out, R.kink, R.t_diff,
                 [R.regimes[br] for br in HEADS]))
    return _REFS[(case, state)]


# ------------------------------------------------------------------------------------------------ the HIP run
def labels_for(B, H, W):
    lab = synth.make_labels(LABEL_SEED, B, H, W)
    return {k: torch.from_numpy(v) for k, v in lab.items()}


def hip_heads(sd, precision):
    from model import MonoConDenseHeads
    heads = MonoConDenseHeads(test_config=None)
    heads.load_state_dict({k[5:]: v for k, v in sd.items() if k.startswith("head.")}, strict=True)
    heads = heads.cuda().train()
    heads._rt.set_precision(precision)
    return heads


def hip_run(R, precision):
    """forward_train + the backward of J on the GPU: (maps, buffers with `head.` keys, feat gradient, parameter gradients)"""
    B, H, W = R.shape
    heads = hip_heads(R.sd, precision)
    fc = R.feat.clone().cuda().requires_grad_(True)
    data = {"label": {k: v.cuda() for k, v in labels_for(B, H, W).items()}, "img_metas": {"pad_shape": [(H, W)] * B}}
    t0 = time.time()
    pd, ld = heads.forward_train(fc, data)
    keys = [k for k, _ in netspec.PRED_KEYS]
    torch.autograd.backward([pd[k] for k in keys], [R.Gs[k].cuda() for k in keys])
    torch.cuda.synchronize()
    seconds = time.time() - t0
    grads = {}
    for n, p in heads.named_parameters():
        assert p.grad is not None, n
        grads[n] = p.grad.detach().cpu()
    bufs = {"head." + k: v.detach().cpu() for k, v in heads.state_dict().items()}
    return {k: v.detach().cpu() for k, v in pd.items()}, bufs, fc.grad.detach().cpu(), grads, seconds


def compare(R, precision, tag):
    """every compared tensor against fp64, gated per kind; prints HIP error / yard-stick per kind before it asserts"""
    preds, bufs, gfeat, grads, seconds = hip_run(R, precision)
    floor = f16x2_floor(R) if precision == "f16x2" else {}
    worst, missed, floor_needed = {}, [], []
    for kind, name, got, ref in R.pairs(preds, bufs, gfeat, grads):
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert bool(torch.isfinite(got).all()), name
        e = rel_l2(got, ref)
        allowed = R.gate[kind] + floor.get(name, 0.0) / max(float(ref.double().norm()), 1e-300)
        if e > R.gate[kind]:
            (floor_needed if e <= allowed else missed).append((name, e, R.gate[kind], allowed))
        if kind not in worst or e / allowed > worst[kind][0] / worst[kind][2]:
            worst[kind] = (e, name, allowed)
    assert set(worst) == set(KINDS)
    print("%s (GPU part %.2f s)" % (tag, seconds))
    for kind in KINDS:
        e, name, allowed = worst[kind]
        print("  %-20s HIP %.2e  float32 %.2e  HIP/float32 %6.2f  gate %.2e  %s%s"
              % (kind, e, R.yard[kind], e / max(R.yard[kind], 1e-300), R.gate[kind], name,
                 "" if e <= R.gate[kind] else ("  (within the f16x2 floor: allowed %.2e)" % allowed if e <= allowed else "  <-- MISSED")))
    for name, e, gate, allowed in floor_needed:
        print("  needs the f16x2 operand floor: %s %.2e, gate %.2e, with the floor %.2e" % (name, e, gate, allowed))
    # a parameter the objective does not reach: an exactly zero gradient (J reaches every head parameter, so none today)
    for n, ref in R.r64.grads.items():
        if ref is None:
            assert float(grads[n].abs().max()) == 0.0, n
    for k, v in R.r64.buffers.items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(v), k
    assert not missed, (tag, missed)


# (case, state, precision, MONOCON_HIP_HEAD_DX_FUSE or None for the default)
RUNS = [("b2", "plain", "fp32", None), ("b2", "plain", "f16x2", None),
        ("b9", "plain", "fp32", None), ("b9", "plain", "f16x2", None),
        ("b17", "plain", "fp32", None), ("b17", "plain", "f16x2", None),
        ("b32", "plain", "fp32", None), ("b32", "plain", "f16x2", None), ("b32", "plain", "bf16x3", None),
        ("b32", "attn", "fp32", None), ("b32", "attn", "f16x2", "0"), ("b32", "attn", "f16x2", "1"),
        ("b32", "out", "fp32", None), ("b32", "out", "f16x2", None),
        ("b64", "plain", "fp32", None), ("b64", "plain", "f16x2", "0"), ("b64", "plain", "f16x2", "1")]


@pytest.mark.parametrize("case,state,precision,fuse", RUNS,
                         ids=["%s-%s-%s%s" % (c, s, p, "" if f is None else "-fuse" + f) for c, s, p, f in RUNS])
def test_head_train_step_vs_fp64(cond_sd, case, state, precision, fuse, monkeypatch):
    """the ten maps, the AttnBN running buffers after one step, the gradient of feat and of every head parameter under the
    map-term objective, each against fp64 within 5 x the float32 oracle's own error of the kind + 4 x 2^-24:

      b2   2 x 96x320    BN(10) over two samples; 60 patches per image: inst_stats_kernel's main loop for parts 0..11, its
                         tail alone for the others; 32 rows per workgroup
      b9   9 x 64x128    the second prefetch group holds one image and seven clamped slots
      b17  17 x 32x64    image 16 wraps the 16-row-group loop; a third prefetch group of one; 4 patches per image
      b32  32 x 32x64    the batch the product trains at; plain, attention-stressed (all three regimes of the hard sigmoid
                         in every head) and output-stressed (both clamps, the depth transform's steep end)
      b64  64 x 32x992   the ABI maximum; 16 workgroups of 124 rows per image: blocks that straddle two 64-pixel tiles;
                         62 patches per image

    MONOCON_HIP_HEAD_DX_FUSE 0 (head_bwd_kernel MODE 0 + the affine pass) and 1 (MODE 1 + head_dx) where listed."""
    assert_partition(case)
    if fuse is not None:
        monkeypatch.setenv("MONOCON_HIP_HEAD_DX_FUSE", fuse)          # read when the train plan is built
    R = reference(cond_sd, case, state)
    R.check_conditions()
    compare(R, precision, "%s/%s %s%s" % (case, state, precision, "" if fuse is None else " DX_FUSE=" + fuse))


# ------------------------------------------------------------------------------------------------ the loss objective at B = 32
def test_loss_objective_at_the_training_batch(cond_sd):
    """sum(losses) through forward_train / backward at B = 32 (32x64): the non-USER pack and the tile map at the batch the
    product trains at, against autograd through the oracle's head in fp64 at the bounds of test_heads_forward_train_standalone
    (losses 1e-4, feat gradient 1e-3, parameters 2e-3).  The losses put their gradient on whatever pixel an object sits on, so
    the hidden ReLU's near-threshold decisions cannot be left out here and a flipped one moves a gradient by ~1e-4: a tighter
    bound would measure the flips, not the kernels (the map-term tests above are the tight ones)."""
    from oracle import monocon_oracle as O
    assert_partition("b32")
    B, H, W = SHAPES["b32"]
    lab = labels_for(B, H, W)
    feat = make_feat(5, B, H, W)
    sd64 = {k: (v.double().clone() if v.dtype == torch.float32 else v.clone()) for k, v in cond_sd.items() if k.startswith("head.")}
    for k, v in sd64.items():
        if v.dtype == torch.float64 and "running" not in k:
            v.requires_grad_(True)
    f64 = feat.double().clone().requires_grad_(True)
    preds = O.head_predictions(O._Ctx(sd64, True), f64)
    L = O.losses(preds, O.make_targets(lab, (H, W), tuple(f64.shape)))
    sum(L.values()).backward()
    heads = hip_heads(cond_sd, "fp32")
    fc = feat.clone().cuda().requires_grad_(True)
    data = {"label": {k: v.cuda() for k, v in lab.items()}, "img_metas": {"pad_shape": [(H, W)] * B}}
    pd, ld = heads.forward_train(fc, data)
    assert list(ld.keys()) == list(netspec.LOSS_KEYS)
    for k, v in ld.items():
        ref = float(L[k].detach())
        assert abs(float(v.detach()) - ref) <= 1e-4 * abs(ref) + 1e-7, (k, float(v.detach()), ref)
    sum(ld.values()).backward()
    torch.cuda.synchronize()
    e = rel_l2(fc.grad, f64.grad)
    print("B = 32 loss objective: feat gradient %.2e" % e)
    assert e < 1e-3, e
    errs = {}
    for n, p in heads.named_parameters():
        ref = sd64["head." + n].grad
        assert p.grad is not None and ref is not None, n
        errs[n] = rel_l2(p.grad, ref)
    worst = max(errs, key=errs.get)
    print("B = 32 loss objective: parameters max %.2e (%s) median %.2e" % (errs[worst], worst, float(np.median(list(errs.values())))))
    assert errs[worst] < 2e-3, (worst, errs[worst])
