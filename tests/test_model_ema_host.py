"""solver.ModelEMA without a device: the decay schedule, the state round trip, ``applied()``'s bit-exact restore, the refusal
to average on the CPU (libmonocon_hip has no CPU path, and there is no torch fall-back), and the SOLVER.EMA config keys."""
import pytest
import torch


def small_model(seed=0):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.BatchNorm2d(5), torch.nn.Linear(4, 3))
    with torch.no_grad():
        m[1].running_mean.normal_()
        m[1].running_var.uniform_(0.5, 2.0)
        m[1].num_batches_tracked.fill_(seed + 3)
    return m


def snapshot(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def same_bits(a, b):
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("t", (0, 1, 9, 10 ** 4))
def test_decay_at(t):
    from solver import ModelEMA
    m = small_model()
    warm, flat = ModelEMA(m, decay=0.9998, warmup=True), ModelEMA(m, decay=0.9998, warmup=False)
    assert flat.decay_at(t) == 0.9998
    assert warm.decay_at(t) == min(0.9998, (1 + t) / (10 + t))
    # the four values spelled out: the warm-up rules until (1 + t) / (10 + t) passes the decay (t > 44989)
    want = {0: 0.1, 1: 2 / 11, 9: 10 / 19, 10 ** 4: 10001 / 10010}[t]
    assert warm.decay_at(t) == want and want < 0.9998
    assert ModelEMA(m, decay=0.5, warmup=True).decay_at(t) == min(0.5, want)
    assert warm.decay_at(10 ** 6) == 0.9998


def test_constructor_copies_the_state_and_checks_decay():
    from solver import ModelEMA
    m = small_model()
    ema = ModelEMA(m)
    assert (ema.decay, ema.warmup, ema.updates) == (0.9998, True, 0)
    assert same_bits(dict(ema.tensors), snapshot(m))
    live = m.state_dict()
    assert all(ema.tensors[k].data_ptr() != live[k].data_ptr() for k in live)
    assert ema.tensors["1.num_batches_tracked"].dtype == torch.int64
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ModelEMA(m, decay=bad)


def test_state_dict_round_trip():
    from solver import ModelEMA
    a = ModelEMA(small_model(1), decay=0.99, warmup=False)
    a.updates = 17
    state = a.state_dict()
    assert set(state) == {"tensors", "updates", "decay", "warmup"}
    b = ModelEMA(small_model(2))
    assert not same_bits(dict(a.tensors), dict(b.tensors))
    ptrs = {k: v.data_ptr() for k, v in b.tensors.items()}
    b.load_state_dict(state)
    assert same_bits(dict(a.tensors), dict(b.tensors))
    assert (b.updates, b.decay, b.warmup) == (17, 0.99, False)
    assert ptrs == {k: v.data_ptr() for k, v in b.tensors.items()}       # in place: a bound table stays valid
    # the loaded average is a copy, not the other one's storage
    b.tensors["0.weight"].add_(1.0)
    assert not torch.equal(a.tensors["0.weight"], b.tensors["0.weight"])
    # through torch.save / torch.load, as a checkpoint carries it
    import io
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    c = ModelEMA(small_model(3))
    c.load_state_dict(torch.load(buf, weights_only=False))
    assert same_bits(dict(a.tensors), dict(c.tensors)) and c.updates == 17
    bad = dict(state, tensors={k: v for k, v in state["tensors"].items() if k != "0.bias"})
    with pytest.raises(KeyError):
        c.load_state_dict(bad)


@pytest.mark.parametrize("raises", (False, True))
def test_applied_restores_every_tensor_bit_for_bit(raises):
    from solver import ModelEMA
    m = small_model(4)
    ema = ModelEMA(small_model(5))
    ema.model = m
    before, avg = snapshot(m), snapshot(small_model(5))
    versions = {k: v._version for k, v in m.state_dict().items()}
    seen = {}

    def body():
        with ema.applied(m) as inside:
            assert inside is m
            seen.update(snapshot(m))
            versions_in = {k: v._version for k, v in m.state_dict().items()}
            assert all(versions_in[k] > versions[k] for k in versions)          # the packed-weight cache's signal, way in
            versions.update(versions_in)
            if raises:
                raise RuntimeError("body failed")

    if raises:
        with pytest.raises(RuntimeError, match="body failed"):
            body()
    else:
        body()
    assert same_bits(seen, avg)                                  # inside: the averaged state, integer entries included
    assert same_bits(snapshot(m), before)                        # outside: the live state, bit for bit
    assert all(v._version > versions[k] for k, v in m.state_dict().items())     # ... and on the way out
    assert same_bits(dict(ema.tensors), avg)                     # the average itself is untouched


def test_copy_to():
    from solver import ModelEMA
    m = small_model(6)
    ema = ModelEMA(small_model(7))
    ema.copy_to(m)
    assert same_bits(snapshot(m), dict(ema.tensors))


def test_update_on_cpu_tensors_raises():
    from hipmonocon.lib import MonoconHipError
    from solver import ModelEMA
    m = small_model(8)
    ema = ModelEMA(m)
    with torch.no_grad():
        m[0].weight.add_(1.0)
        m[1].num_batches_tracked.add_(1)
    before = snapshot_of(ema)
    with pytest.raises(MonoconHipError):
        ema.update(m)
    assert ema.updates == 0 and same_bits(snapshot_of(ema), before)      # nothing averaged, copied or counted


def snapshot_of(ema):
    return {k: v.clone() for k, v in ema.tensors.items()}


def test_solver_ema_defaults():
    from utils.engine_utils import get_default_cfg
    c = get_default_cfg()
    assert c.SOLVER.EMA.ENABLE is False
    assert c.SOLVER.EMA.DECAY == 0.9998 and c.SOLVER.EMA.WARMUP is True
    assert set(c.SOLVER.EMA.keys()) == {"ENABLE", "DECAY", "WARMUP"}


def test_infer_raw_use_ema_loads_the_averaged_weights(tmp_path, monkeypatch):
    """``infer_raw.py --use_ema`` hands test_raw.py's ``main`` a detector class whose ``load_checkpoint`` takes the checkpoint's
    ``state_dict['ema']``; a file without one is an error.  test_raw's main itself is stood in for: it needs a device."""
    import os
    import sys
    import infer_raw
    import model.detector as detector_pkg
    import test_raw
    from model import MonoConDetector
    torch.manual_seed(0)
    live = MonoConDetector(34, pretrained_backbone=False)
    avg = {k: (v + 1 if v.is_floating_point() else v + 7) for k, v in live.state_dict().items()}
    with_ema, without = os.path.join(tmp_path, "ema.pth"), os.path.join(tmp_path, "plain.pth")
    base = {'model': live.state_dict(), 'optimizer': None, 'scheduler': None}
    torch.save({'engine_attrs': {}, 'state_dict': base}, without)
    torch.save({'engine_attrs': {}, 'state_dict': dict(base, ema={'tensors': avg, 'updates': 3, 'decay': 0.9, 'warmup': True})},
               with_ema)
    seen = {}
    monkeypatch.setattr(detector_pkg, "MonoConDetector", detector_pkg.MonoConDetector)      # (restored afterwards)
    monkeypatch.setattr(test_raw, "main", lambda: seen.update(cls=detector_pkg.MonoConDetector, argv=list(sys.argv)))
    monkeypatch.setattr(sys, "argv", ["infer_raw.py", "--use_ema", "--checkpoint_file", with_ema])
    infer_raw.main()
    assert seen["argv"] == ["infer_raw.py", "--checkpoint_file", with_ema]      # the flag is infer_raw's own
    assert issubclass(seen["cls"], MonoConDetector) and seen["cls"] is not MonoConDetector
    det = seen["cls"](pretrained_backbone=False)
    det.load_checkpoint(with_ema)                   # as test_raw.py calls it
    assert all(torch.equal(v, avg[k]) for k, v in det.state_dict().items())
    with pytest.raises(KeyError, match="no averaged weights"):
        det.load_checkpoint(without)
    plain = MonoConDetector(34, pretrained_backbone=False)
    plain.load_checkpoint(with_ema)                 # without the flag: the live weights, as before
    assert all(torch.equal(v, live.state_dict()[k]) for k, v in plain.state_dict().items())
    with pytest.raises(KeyError, match="no averaged weights"):
        plain.load_checkpoint(without, use_ema=True)
