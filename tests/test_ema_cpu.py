"""The weight average (TrainSession(ema_decay=...)) without a GPU: the specification's own properties, the configuration key, the argument
checks of yolo2_ema_update and both checkpoint containers on the host."""
import os
import tempfile

import numpy as np
import pytest

import ema_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decay_schedule_is_tensorflows_num_updates_rule():
    assert ema_ref.decay_at(0.999, 1) == 2 / 11
    d = [ema_ref.decay_at(0.999, t) for t in range(1, 9200)]
    assert all(b >= a for a, b in zip(d, d[1:]))
    # (1 + t) / (10 + t) >= 0.999  <=>  t >= 8990
    assert ema_ref.decay_at(0.999, 8989) < 0.999
    assert all(ema_ref.decay_at(0.999, t) == 0.999 for t in range(8990, 9200))
    assert all(ema_ref.decay_at(0.5, t) == 0.5 for t in range(8, 200))
    assert [ema_ref.decay_at(0.5, t) for t in range(1, 8)] == [(1.0 + t) / (10.0 + t) for t in range(1, 8)]


def test_product_schedule_equals_the_specification():
    from yolo_tf_amd.session import ema_decay_at
    for decay in (0.5, 0.9, 0.999, 0.9999):
        for t in list(range(1, 40)) + [8989, 8990, 8991, 10 ** 6]:
            assert ema_decay_at(decay, t) == ema_ref.decay_at(decay, t)


def test_update_end_points():
    """one_minus_decay = 0 leaves the shadows as they are, bit for bit.  one_minus_decay = 1 gives e - fl(e - w): the inner difference is off by at most
    half an ulp of itself and the outer one by half an ulp of the result, both of magnitude <= |e| + |w| -- so the result lies within one f32 ulp at
    that magnitude of w.  Exact equality is not promised by the three-rounding rule."""
    rng = np.random.RandomState(0)
    e = (rng.randn(4096) * rng.choice([1e-3, 1.0, 1e3], 4096)).astype(np.float32)
    w = (rng.randn(4096) * rng.choice([1e-3, 1.0, 1e3], 4096)).astype(np.float32)
    same = ema_ref.update(e, w, 0.0)
    assert same.dtype == np.float32 and np.array_equal(same.view(np.int32), e.view(np.int32))
    full = ema_ref.update(e, w, 1.0)
    ulp = np.spacing(np.abs(e) + np.abs(w))
    assert np.all(np.abs(full.astype(np.float64) - w.astype(np.float64)) <= ulp.astype(np.float64))
    # NaN and inf propagate; a shadow equal to its variable stays put whatever the decay
    special = ema_ref.update(np.float32([np.nan, 1, np.inf, -np.inf, 2.5]), np.float32([1, np.nan, 1, 1, 2.5]), 0.25)
    assert np.isnan(special[0]) and np.isnan(special[1]) and np.isnan(special[2]) and np.isnan(special[3]) and special[4] == 2.5


def test_run_starts_at_the_initial_parameters():
    w0 = np.float32([1.0, -2.0])
    hist = [np.float32([2.0, -2.0]), np.float32([3.0, 0.0])]
    out = ema_ref.run(w0, hist, 0.5)
    e1 = ema_ref.update(w0, hist[0], np.float32(1.0 - 2 / 11))
    e2 = ema_ref.update(e1, hist[1], np.float32(1.0 - 3 / 12))
    assert len(out) == 2 and np.array_equal(out[0], e1) and np.array_equal(out[1], e2)
    assert w0[0] == 1.0                                                # the caller's array is not written


def _config(value):
    """The product configuration of the tiny network, as tests/test_quant_cpu.py builds it, with ``[mi355x] ema_decay = value`` (None: absent)."""
    from yolo_tf_amd import utils
    with tempfile.TemporaryDirectory() as basedir:
        cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo2', 'tiny-20.ini')], basedir)
    if not cfg.has_section('mi355x'):
        cfg.add_section('mi355x')
    cfg.remove_option('mi355x', 'ema_decay')
    if value is not None:
        cfg.set('mi355x', 'ema_decay', value)
    return cfg


def test_config_key_absent_zero_on_and_out_of_range():
    """TrainSession builds an Engine, which needs the GPU: this tests ``session.ema_decay_option``, the helper TrainSession.__init__ calls first with
    its ``ema_decay`` argument and its configuration (tests/test_ema_gpu.py covers the session's own behaviour)."""
    from yolo_tf_amd.session import ema_decay_option
    assert ema_decay_option(None, _config(None)) == 0.0                 # absent: off
    assert ema_decay_option(None, _config('0')) == 0.0                  # 0: off
    assert ema_decay_option(None, _config('0.999')) == 0.999            # on
    for bad in ('1.0', '-0.1'):
        with pytest.raises(ValueError, match='ema_decay'):
            ema_decay_option(None, _config(bad))
    # the argument wins over the key; no configuration at all is off
    assert ema_decay_option(0.5, _config('0.999')) == 0.5 and ema_decay_option(0, _config('0.999')) == 0.0
    assert ema_decay_option(None, None) == 0.0
    for bad in (1.0, -0.1, float('nan'), 2):
        with pytest.raises(ValueError, match='ema_decay'):
            ema_decay_option(bad, None)


def test_shipped_configuration_leaves_the_average_off():
    from yolo_tf_amd import utils
    from yolo_tf_amd.session import ema_decay_option
    with tempfile.TemporaryDirectory() as basedir:
        for ini in ('tiny-20.ini', 'darknet-20.ini'):
            cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo2', ini)], basedir)
            assert ema_decay_option(None, cfg) == 0.0


def test_ema_update_argument_errors_raise_without_touching_the_gpu():
    from yolo_tf_amd import _lib
    ok = 1 << 20                                                    # a 16-byte aligned, never dereferenced address
    for args in [(None, ok, 16, 0.5, None), (ok, None, 16, 0.5, None), (ok, ok, 0, 0.5, None), (ok, ok, -4, 0.5, None),
                 (ok, ok, 16, 1.5, None), (ok, ok, 16, -0.1, None), (ok, ok, 16, float('nan'), None)]:
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            _lib.call('yolo2_ema_update', *args)


# ---------------------------------------------------------------------------------------------------------------------
# both checkpoint containers, on the host (the stand-ins of tests/test_tf_formats_cpu.py with the session's three EMA members)
# ---------------------------------------------------------------------------------------------------------------------
def _session(ema):
    import torch
    from test_tf_formats_cpu import _FakeSession
    s = _FakeSession()
    e = s.engine
    s.ema, s.ema_var = None, {}

    def reset_ema():
        for name, (o, n) in e.param_offsets.items():
            s.ema[o:o + n].copy_(torch.from_numpy(np.ascontiguousarray(e.values[name], np.float32).reshape(-1)))
    s.reset_ema = reset_ema
    if ema:
        s.ema = torch.arange(e.n, dtype=torch.float32) * 0.5 - 3.0
        s.ema_var = {name: s.ema[o:o + n] for name, (o, n) in e.param_offsets.items()}
    return s


def _shadow_arrays(s):
    e = s.engine
    host = s.ema.numpy()
    return {v.name: host[e.param_offsets[v.name][0]:e.param_offsets[v.name][0] + v.size].reshape(v.shape).copy() for v in e.graph.trainable()}


@pytest.mark.parametrize('container', ['npz', 'tf'])
def test_checkpoint_containers_carry_the_shadows(tmp_path, container, caplog):
    import torch
    from yolo_tf_amd import checkpoint, tf_checkpoint
    C = checkpoint if container == 'npz' else tf_checkpoint
    donor = _session(ema=True)
    donor.global_step = 12
    want = _shadow_arrays(donor)
    raw = donor.engine.get_variables()
    trainable = [v.name for v in donor.engine.graph.trainable()]
    path = C.save(str(tmp_path / 'on'), donor)
    plain = _session(ema=False)
    plain.global_step = 12
    path_plain = C.save(str(tmp_path / 'off'), plain)
    if container == 'tf':
        index = tf_checkpoint.read_index(path)
        assert sorted(k for k in index if k.endswith('/ExponentialMovingAverage')) == sorted(n + '/ExponentialMovingAverage' for n in trainable)
        assert not [k for k in tf_checkpoint.read_index(path_plain) if 'ExponentialMovingAverage' in k]
        tensors = tf_checkpoint.read(path)
        for n in trainable:
            assert np.array_equal(tensors[n + '/ExponentialMovingAverage'], want[n]) and np.array_equal(tensors[n], raw[n])
    else:
        z, zp = np.load(path), np.load(path_plain)
        assert set(z.files) - set(zp.files) == {'ema'} and set(zp.files) <= set(z.files)
        assert np.array_equal(z['ema'], donor.ema.numpy())
    # a full resume into a session that keeps the average: the shadows come back
    s = _session(ema=True)
    s.ema.zero_()
    assert C.restore(path, s) == 12
    assert torch.equal(s.ema, donor.ema)
    # a file without shadows, and a transfer: the shadows are the restored parameters, with one warning each
    for p, kw in ((path_plain, {}), (path, dict(variables_only=True))):
        s = _session(ema=True)
        caplog.clear()
        C.restore(p, s, **kw)
        got = _shadow_arrays(s)
        assert all(np.array_equal(got[n], raw[n]) for n in trainable)
        assert len([r for r in caplog.records if 'moving averages' in r.getMessage()]) == 1
    # a session without the average ignores them
    s = _session(ema=False)
    C.restore(path, s)
    assert s.ema is None and all(np.array_equal(s.engine.values[n], raw[n]) for n in trainable)
    # the inference form: ema=True assigns the shadows to the trainable variables (and nothing else), ema=False the raw values
    from test_tf_formats_cpu import _FakeEngine
    e = _FakeEngine()
    C.restore(path, engine=e, ema=True)
    for v in e.graph.variables.values():
        assert np.array_equal(e.values[v.name], want[v.name] if v.name in trainable else raw[v.name]), v.name
    e = _FakeEngine()
    C.restore(path, engine=e, ema=False)
    assert all(np.array_equal(e.values[n], raw[n]) for n in raw)
    with pytest.raises(SystemExit) as exc:
        C.restore(path_plain, engine=_FakeEngine(), ema=True)
    assert str(path_plain) in str(exc.value) and '[mi355x] ema_decay' in str(exc.value)


def test_npz_shadows_follow_moved_arena_offsets(tmp_path):
    """Same variables at other offsets: the shadows are moved variable by variable, as the optimizer slots are."""
    import torch
    from yolo_tf_amd import checkpoint
    donor = _session(ema=True)
    path = checkpoint.save(str(tmp_path), donor)
    s = _session(ema=True)
    e = s.engine
    pad, off = 8, 0
    for name, (_, n) in list(e.param_offsets.items()):
        e.param_offsets[name] = (off + pad, n)
        off += n + pad
    s.ema = torch.full((off + pad,), -1.0)
    s.optimizer.slots = [torch.zeros(off + pad), torch.zeros(off + pad)]
    checkpoint.restore(path, s)
    for name, (o, n) in e.param_offsets.items():
        do, _ = donor.engine.param_offsets[name]
        assert torch.equal(s.ema[o:o + n], donor.ema[do:do + n]), name
