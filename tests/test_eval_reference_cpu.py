"""The layer-local eval reference of `plan_graph.py` checked against the oracle, without a GPU.

1. Chained on its own outputs in float64 (`eval_conv`, max_pool2d, `eval_deconv`, `head_hidden`, `attn_affine`,
   `head_outputs`), the reference reproduces `O.forward(sd, img, train=False)` run in float64: every level, `feat` and the ten
   maps, norm-wise.  Measured on the golden and on the stressed state at 1x64x64: <= 5.1e-14 (depth row 0); bound 1e-12.  `attn_affine`'s
   scale x + shift equals the oracle's `_attn_bn`.
2. The gates of the GPU file (`evaluate_eval`) are run on a float32 stand-in for the kernels: the eval forward in float32 with
   the BatchNorm FOLDED (scale = gamma / sqrt(rv + eps), shift = beta - rm scale), as the conv epilogue applies it.  (torch's
   CPU F.batch_norm folds too: most layers come out bit-equal to the yard-stick, the rest within 1.2 x.)  It passes every class
   on both states.
3. Three negative controls: the same stand-in with ONE defect must fail, in the class the defect belongs to:
       one BatchNorm folded with shift = beta + rm scale        -> its conv kind
       one root conv with two of its sources swapped            -> 1x1
       AttnBN with the biased variance                          -> AttnBN
   and nothing downstream of the defect may fail with it (the reference is layer-local).
4. `head_output_stress` puts >= 5 % of both heat maps at the floor, at the ceiling and in the interior in the fp64 reference
   (measured at 2x64x128 with gain 12: see test_head_output_stress_reaches_both_clamps), and the depth logit within +-30.
"""
import pytest
import torch
import torch.nn.functional as F

from plan_graph import (EPS, EVAL_KINDS, HEADS, HEAT_KEYS, LOGIT_CLAMP, STEM_REC, attn_affine, eval_conv, eval_deconv,
                        eval_reference, evaluate_eval, head_hidden, head_output_stress, head_outputs, norm_err, plan_graph,
                        stressed_batch, stressed_state_dict)

B, H, W = 1, 64, 64
CHAIN_TOL = 1e-12
BN_DEFECT = "backbone.level3.tree1.tree1.conv2"
ROOT_DEFECT = "backbone.level3.tree2.root.conv"


def _inputs(golden_sd, state):
    from hipmonocon import synth
    if state == "stressed":
        return stressed_state_dict(golden_sd), stressed_batch(77, B, H, W)["img"]
    return golden_sd, synth.make_batch(77, B, H, W, with_labels=False)["img"]


def _forward(sd, G, img, dtype, folded=False, defect=None):
    """the eval forward chained on its own outputs.  folded: BatchNorm as scale / shift in `dtype`, as the conv epilogue applies
    it; defect: None / "bn" / "root" / "attn" (see the module docstring).  -> nodes (with the image as node -1), hidden,
    attn (B, 2, 9, 64), maps"""
    nodes = {-1: img.to(dtype)}

    def bn_of(name):
        def bn(y, g, b, rm, rv):
            scale = g / torch.sqrt(rv + EPS)
            shift = b + rm * scale if (defect == "bn" and name == BN_DEFECT) else b - rm * scale
            return y * scale[None, :, None, None] + shift[None, :, None, None]
        return bn if folded else None

    for st in [("conv", STEM_REC)] + list(G.steps):
        if st[0] == "pool":
            nodes[st[2]] = F.max_pool2d(nodes[st[1]], 2)
        elif st[0] == "deconv":
            nodes[st[3]] = eval_deconv(sd, st[1], nodes[st[2]], dtype)
        else:
            rec = st[1]
            if defect == "root" and rec[0] == ROOT_DEFECT:
                srcs = list(rec[1])
                assert G.node_c[srcs[0]] == G.node_c[srcs[1]] and srcs[0] != srcs[1]
                srcs[0], srcs[1] = srcs[1], srcs[0]
                rec = (rec[0], srcs) + tuple(rec[2:])
            nodes[rec[4]] = eval_conv(sd, rec, nodes, dtype, bn_of(rec[0]))
    hidden = head_hidden(sd, nodes[G.feat], dtype)
    a = attn_affine(sd, hidden, dtype, biased=(defect == "attn"))
    attn = torch.stack([a["scale"], a["shift"]], 1)
    maps = head_outputs(sd, hidden, attn[:, 0], attn[:, 1], dtype)[1]
    return nodes, hidden, attn, maps


@pytest.fixture(scope="module")
def graph():
    return plan_graph()


@pytest.mark.parametrize("state", ["golden", "stressed"])
def test_chained_reference_reproduces_the_oracle_in_float64(golden_sd, graph, state):
    from oracle import monocon_oracle as O
    sd, img = _inputs(golden_sd, state)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        ref, feat, levels, _ = O.forward(sd64, img.double(), train=False, return_levels=True)
        nodes, hidden, attn, maps = _forward(sd, graph, img, torch.float64)
        errs = {"l%d" % i: norm_err(nodes[n], levels[i]) for i, n in enumerate(graph.levels)}
        errs["feat"] = norm_err(nodes[graph.feat], feat)
        for k in ref:
            assert maps[k].shape == ref[k].shape, k
            errs[k] = norm_err(maps[k], ref[k])
        # AttnBN as one affine per (image, channel) is the oracle's _attn_bn
        cx = O._Ctx(sd64, False)
        for hd, head in enumerate(HEADS):
            x = hidden[:, 64 * hd:64 * hd + 64]
            y = x * attn[:, 0, hd, :, None, None] + attn[:, 1, hd, :, None, None]
            errs["attn " + head] = norm_err(y, O._attn_bn(cx, x, "head.%s.1" % head))
    print("\n[eval reference] %s: chained fp64 reference against the fp64 oracle, worst %.3g (%s)"
          % (state, max(errs.values()), max(errs, key=errs.get)))
    bad = {k: v for k, v in errs.items() if not v <= CHAIN_TOL}
    assert not bad, bad


def _evaluate(sd, G, img, defect):
    with torch.no_grad():
        nodes, hidden, attn, maps = _forward(sd, G, img, torch.float32, folded=True, defect=defect)
        R = eval_reference(sd, G, nodes, hidden, attn)
        return evaluate_eval(R, nodes, hidden, attn, maps)


@pytest.fixture(scope="module")
def clean(golden_sd, graph):
    out = {}
    for state in ("golden", "stressed"):
        sd, img = _inputs(golden_sd, state)
        out[state] = _evaluate(sd, graph, img, None)
    return out


@pytest.mark.parametrize("state", ["golden", "stressed"])
def test_a_float32_forward_with_folded_batchnorm_passes_every_gate(clean, state):
    Fg = clean[state]
    for cls in list(EVAL_KINDS) + ["AttnBN", "linear rows", "heat maps", "depth row 0"]:
        print("\n[eval reference] %s %-12s stand-in %.3g / float32 %.3g = %.2f" % (state, cls, Fg.worst[cls], Fg.yard[cls], Fg.ratio(cls)))
    assert not any(Fg.bad.values()), Fg.bad
    assert max(Fg.excepted.values()) == 0.0, Fg.excepted          # (no position needed the exception near a clamp)


@pytest.mark.parametrize("state", ["golden", "stressed"])
@pytest.mark.parametrize("defect,cls", [("bn", "3x3s1"), ("root", "1x1"), ("attn", "AttnBN")])
def test_negative_controls_fail_where_the_defect_is(golden_sd, graph, state, defect, cls):
    sd, img = _inputs(golden_sd, state)
    Fg = _evaluate(sd, graph, img, defect)
    failed = sorted(k for k, v in Fg.bad.items() if v)
    print("\n[eval reference] %s defect %-4s fails %s: %s" % (state, defect, failed, Fg.bad[cls][:1]))
    assert failed == [cls], Fg.bad
    name = {"bn": BN_DEFECT, "root": ROOT_DEFECT, "attn": "scale"}[defect]
    assert any(name in line for line in Fg.bad[cls]), Fg.bad[cls]
    if defect != "attn":
        assert len(Fg.bad[cls]) == 1, Fg.bad[cls]          # the one layer, nothing downstream of it


def test_head_output_stress_reaches_both_clamps(golden_sd, graph):
    """the inputs of the GPU file's head-output stress, in the fp64 reference: floor / ceiling / interior each >= 5 % of both
    heat maps, |raw depth logit| <= 30.  Measured (gain 12, depth gain 6, feat of the golden forward at 2x64x128): see the
    printed line; the GPU test asserts the same shares on its own reference."""
    from hipmonocon import synth
    img = synth.make_batch(5400, 2, 64, 128, with_labels=False)["img"]
    with torch.no_grad():
        nodes, hidden, attn, _ = _forward(golden_sd, graph, img, torch.float64)
        sd = head_output_stress(golden_sd, 12.0, 6.0)
        raw, out, _ = head_outputs(sd, hidden, attn[:, 0], attn[:, 1], torch.float64)
    for key in HEAT_KEYS:
        sh = heat_shares(raw[key])
        print("\n[eval reference] head output stress %s: floor %.1f %%, ceiling %.1f %%, interior %.1f %%"
              % ((key,) + tuple(100 * s for s in sh)))
        assert min(sh) >= 0.05, (key, sh)
    d = raw["depth_pred"][:, 0]
    print("\n[eval reference] head output stress depth logit [%.2f, %.2f], d0 [%.3g, %.3g]"
          % (float(d.min()), float(d.max()), float(out["depth_pred"][:, 0].min()), float(out["depth_pred"][:, 0].max())))
    assert float(d.abs().max()) <= 30 and float(d.max()) > 15 and float(d.min()) < -15


def heat_shares(raw):
    """(floor, ceiling, interior) shares of a heat map from its fp64 raw logits"""
    lo, hi = float((raw <= -LOGIT_CLAMP).double().mean()), float((raw >= LOGIT_CLAMP).double().mean())
    return lo, hi, 1.0 - lo - hi
