"""TrainSession(accum_steps=, weight_decay=, weight_decay_mode=) on the device: what a micro-batch may and may not change, the whole update
against the NumPy specification (tests/grad_combine_ref.py) bit for bit, off is off, the weight average once per update, the refusals, two ranks on one GPU.
`tiny-20` at 64 x 64, batch 2, K = 3 (so that f32(1 / K) is inexact)."""
import os
import tempfile

import numpy as np
import pytest
import torch

import ema_ref
import grad_combine_ref as ref
from test_network_gpu import make_builder

pytestmark = pytest.mark.gpu

K, B, SIZE, WD, LR = 3, 2, 64, 5e-4, 1e-3


@pytest.fixture(scope='module')
def basedir():
    with tempfile.TemporaryDirectory() as d:
        yield d


@pytest.fixture(scope='module')
def builder(basedir):
    return make_builder('tiny', 20, SIZE, True, basedir)[0]


_BATCHES = {}


def _batch(i):
    """Micro-batch i: fixed images and labels, made once."""
    if i not in _BATCHES:
        from yolo_tf_amd.utils import data
        images = torch.rand(B, SIZE, SIZE, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(10 + i)) * 255
        _BATCHES[i] = (images, data.synthetic_batch(B, 20, SIZE // 32, SIZE // 32, seed=20 + i))
    return _BATCHES[i]


def _session(builder, **kw):
    from yolo_tf_amd.session import TrainSession
    kw.setdefault('optimizer', 'adam')
    return TrainSession(builder, B, dtype='f32', learning_rate=LR, seed=4, **kw)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def test_structure_of_an_update_in_the_default_mode(builder):
    sess = _session(builder, accum_steps=K)
    e = sess.engine
    assert sess.accum_steps == K and sess.micro_step == 0 and sess.global_step == 0 and sess.weight_decay == 0.0 and sess.decay_table is None
    assert sess.grad_acc.dtype == torch.float32 and sess.grad_acc.numel() == e.n_params and sess.grad_acc.data_ptr() not in (e.grads.data_ptr(), e.params.data_ptr())
    assert not sess.early_adam
    for i in range(2 * K):
        params, slots, state = e.params.clone(), [s.clone() for s in sess.optimizer.slots], e.state.clone()
        sess.step(*_batch(i))
        torch.cuda.synchronize()
        assert not _same(e.state, state), i                              # the BN moving statistics follow every micro-batch
        assert sess.micro_step == (i + 1) % K and sess.global_step == (i + 1) // K
        updated = (i + 1) % K == 0
        assert _same(e.params, params) != updated, i                     # parameters and optimizer slots keep their bits until the K-th call
        assert all(_same(a, b) != updated for a, b in zip(sess.optimizer.slots, slots)), i
    out = sess.fetch()
    assert np.isfinite(out['total_loss'])
    with pytest.raises(AssertionError, match='micro-batch'):
        sess.apply_gradients()                                           # no update is due


CHAIN = [
    pytest.param('adam', 0.0, 'l2', id='adam-fused-l2'),
    pytest.param('adam', 0.0, 'decoupled', id='adam-fused-decoupled'),
    pytest.param('momentum', 0.0, 'l2', id='momentum-l2'),
    pytest.param('momentum', 0.0, 'decoupled', id='momentum-decoupled'),
    pytest.param('adam', 5.0, 'l2', id='adam-clip5-l2'),
    pytest.param('momentum', 5.0, 'decoupled', id='momentum-clip5-decoupled'),
]


@pytest.mark.parametrize('optimizer,clip,mode', CHAIN)
def test_an_update_equals_the_specification_bit_for_bit(builder, optimizer, clip, mode):
    """Session A accumulates K micro-batches with weight decay.  Session B, the plain session with the same seed, runs forward_backward on the same
    micro-batches; the specification combines B's K gradients with B's parameters; the result goes into B's gradient arena (the shrunk filters into its
    parameters) and B applies it.  Two updates, so that the second one's STORE meets an accumulator that is in use."""
    a = _session(builder, optimizer=optimizer, gradient_clip=clip, deterministic=True, accum_steps=K, weight_decay=WD, weight_decay_mode=mode)
    b = _session(builder, optimizer=optimizer, gradient_clip=clip, deterministic=True)
    assert b.grad_acc is None and b.decay_table is None and _same(a.engine.params, b.engine.params)
    ranges = ref.weight_ranges(b.engine.param_offsets)
    assert a.decay_table.cpu().tolist() == [v for r in ranges for v in r]
    for update in range(2):
        grads = []
        for k in range(K):
            images, labels = _batch(K * update + k)
            a.step(images, labels)
            b.upload_labels(labels)
            b.forward_backward(images)
            torch.cuda.synchronize()
            grads.append(b.engine.grads.cpu().numpy().copy())
        decay, shrink = (WD, 1.0) if mode == 'l2' else (0.0, float(np.float32(1.0 - LR * WD)))
        w = b.engine.params.cpu().numpy()
        g, w2 = ref.accumulate(grads, w, decay, shrink, ranges)
        assert np.isfinite(g).all() and not np.array_equal(g, grads[-1])
        b.engine.grads.copy_(torch.from_numpy(g))
        if mode == 'decoupled':
            assert not np.array_equal(w2, w)
            b.engine.params.copy_(torch.from_numpy(w2))
            b.engine._filters_dirty = True
        b.apply_gradients()
        torch.cuda.synchronize()
        assert a.global_step == b.global_step == update + 1 and a.micro_step == 0
        assert _same(a.engine.params, b.engine.params), update
        assert all(_same(x, y) for x, y in zip(a.optimizer.slots, b.optimizer.slots)), update
        assert _same(a.engine.state, b.engine.state), update
    assert len(a.optimizer.slots) == (2 if optimizer == 'adam' else 1)


def test_weight_decay_alone_runs_the_final_launch_without_an_accumulator(builder):
    a = _session(builder, deterministic=True, weight_decay=WD)
    b = _session(builder, deterministic=True)
    assert a.accum_steps == 1 and a.grad_acc is None and a.decay_table is not None
    images, labels = _batch(0)
    a.step(images, labels)
    b.upload_labels(labels)
    b.forward_backward(images)
    torch.cuda.synchronize()
    g, _ = ref.accumulate([b.engine.grads.cpu().numpy()], b.engine.params.cpu().numpy(), WD, 1.0, ref.weight_ranges(b.engine.param_offsets))
    b.engine.grads.copy_(torch.from_numpy(g))
    b.apply_gradients()
    torch.cuda.synchronize()
    assert a.global_step == 1 and a.micro_step == 0 and _same(a.engine.params, b.engine.params)
    assert all(_same(x, y) for x, y in zip(a.optimizer.slots, b.optimizer.slots))


def test_off_is_off(builder):
    absent = _session(builder, deterministic=True)
    explicit = _session(builder, deterministic=True, accum_steps=1, weight_decay=0.0, weight_decay_mode='decoupled')
    for s in (absent, explicit):
        assert s.accum_steps == 1 and s.weight_decay == 0.0 and s.grad_acc is None and s.decay_table is None and s.micro_step == 0
        for i in range(2):
            s.step(*_batch(i))
        assert s.micro_step == 0 and s.global_step == 2
    torch.cuda.synchronize()
    assert _same(absent.engine.params, explicit.engine.params) and _same(absent.engine.state, explicit.engine.state)
    assert all(_same(x, y) for x, y in zip(absent.optimizer.slots, explicit.optimizer.slots))


def test_the_weight_average_follows_once_per_update(builder):
    sess = _session(builder, deterministic=True, accum_steps=K, ema_decay=0.9)
    e = sess.engine
    w0, history, shadows = e.params.clone(), [], []
    for i in range(2 * K):
        before = sess.ema.clone()
        sess.step(*_batch(i))
        torch.cuda.synchronize()
        if sess.micro_step == 0:
            history.append(e.params.cpu().numpy())
            shadows.append(sess.ema.cpu().numpy())
        else:
            assert _same(sess.ema, before)
    want = ema_ref.run(w0.cpu().numpy(), history, 0.9)
    assert len(want) == 2
    for got, r in zip(shadows, want):
        for name, (o, n) in e.param_offsets.items():
            assert np.array_equal(got[o:o + n].view(np.int32), r[o:o + n].view(np.int32)), name
    assert not np.array_equal(shadows[-1], history[-1])


def test_refusals_come_before_any_kernel(builder, basedir, monkeypatch):
    from yolo_tf_amd import _lib
    from yolo_tf_amd.session import TrainSession
    import test_yolo1_gpu
    v1 = test_yolo1_gpu.make_builder(20, 192, True, basedir)

    def no_kernel(name, *args):
        raise AssertionError('%s ran before the refusal' % name)
    monkeypatch.setattr(_lib, 'call', no_kernel)
    monkeypatch.setattr('yolo_tf_amd.ops.call', no_kernel)
    with pytest.raises(NotImplementedError, match='accum_steps'):
        TrainSession(v1, B, dtype='f32', accum_steps=2)
    with pytest.raises(NotImplementedError, match=r'shard_optimizer.*accum_steps'):
        TrainSession(builder, B, dtype='f32', accum_steps=2, shard_optimizer=True)
    with pytest.raises(NotImplementedError, match=r'shard_optimizer.*weight_decay'):
        TrainSession(builder, B, dtype='f32', weight_decay=WD, shard_optimizer=True)
    with pytest.raises(NotImplementedError, match=r'weight_decay_mode = decoupled.*ftrl'):
        TrainSession(builder, B, dtype='f32', optimizer='ftrl', weight_decay=WD, weight_decay_mode='decoupled')
    for kw, key in (({'accum_steps': 0}, 'accum_steps'), ({'weight_decay': -1.0}, 'weight_decay'), ({'weight_decay_mode': 'adamw'}, 'weight_decay_mode')):
        with pytest.raises(ValueError, match=key):
            TrainSession(builder, B, dtype='f32', **kw)
    monkeypatch.undo()
    # the early-update candidate is simply not taken
    monkeypatch.setenv('YOLO2_EARLY_ADAM', '1')
    assert _session(builder).early_adam and not _session(builder, weight_decay=WD).early_adam and not _session(builder, accum_steps=2).early_adam
    # ... and the [mi355x] keys are read where the arguments are None
    import configparser
    cfg = configparser.ConfigParser()
    cfg.read_dict(builder.config)
    if not cfg.has_section('mi355x'):
        cfg.add_section('mi355x')
    cfg.set('mi355x', 'accum_steps', '4')
    cfg.set('mi355x', 'weight_decay', '0.0005')
    s = _session(builder, config=cfg)
    assert (s.accum_steps, s.weight_decay, s.weight_decay_mode) == (4, 0.0005, 'l2') and s.grad_acc is not None
    assert _session(builder, config=cfg, accum_steps=1, weight_decay=0.0).grad_acc is None


def test_two_ranks_on_one_gpu(tmp_path):
    """Data parallel with K = 2 and weight decay: micro-batch 0 is local; the last one runs backward, the final launch, then ONE flush of every bucket.  Both
    ranks end with bitwise identical parameters; the reducer was begun once per update and every bucket left once per update, after the last micro-batch."""
    import socket
    import torch.multiprocessing as mp
    import _train_recipe_worker as W
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(W.worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(str(tmp_path / 'rank0.npz')), np.load(str(tmp_path / 'rank1.npz'))
    for tag in ('deferred', 'clip'):
        for key in ('params', 'slot0'):
            assert np.array_equal(r0['%s/%s' % (tag, key)].view(np.int32), r1['%s/%s' % (tag, key)].view(np.int32)), (tag, key)
        assert not np.array_equal(r0[tag + '/params'], r0[tag + '/w0'])
        for r in (r0, r1):
            assert r[tag + '/begun'].tolist() == [[u, W.K - 1] for u in range(W.UPDATES)], tag
            assert r[tag + '/launched'].tolist() == [[u, W.K - 1] for u in range(W.UPDATES) for _ in range(int(r[tag + '/buckets']))], tag
