"""The weight average on the device: yolo2_ema_update against the NumPy specification (tests/ema_ref.py) bit for bit, the session's recurrence through
every update branch, both checkpoint containers, inference from the shadows, and two data-parallel ranks."""
import itertools
import os

import numpy as np
import pytest
import torch

import ema_ref
from test_network_gpu import ROOT, make_builder

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(12345.0)
SIZES = [1, 3, 255, 256, 257, 1024, 65536 + 3, 2 ** 22 + 5]
OFFSETS = list(itertools.product(range(4), range(4)))                 # (ema, w) element offsets from a 16-byte boundary
OMDS = [0.0, 2.0 ** -10, 0.001, 9.0 / 11.0, 1.0]
SCALES = [1e-3, 1.0, 1e3]
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-41], np.float32)     # (1e-41: a denormal)


@pytest.fixture(scope='module')
def basedir():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        yield d


def _bits_equal_nan_by_position(got, want):
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got.view(np.int32)[~gn], want.view(np.int32)[~wn])


_NOISE = []


def _inputs(n, scale, k):
    """randn x scale with the special values planted: windows of two fixed noise arrays (drawn once), a different window for every case."""
    if not _NOISE:
        rng = np.random.RandomState(5)
        _NOISE.extend(rng.standard_normal(max(SIZES) + 4096).astype(np.float32) for _ in range(2))
    e = _NOISE[0][3 * k:3 * k + n] * np.float32(scale)
    w = _NOISE[1][5 * k:5 * k + n] * np.float32(scale)
    if n >= 16:
        for j, s in enumerate(SPECIALS):
            e[(7 * j + k) % n] = s
            w[(11 * j + 3 + k) % n] = s
    else:               # too short for all of them: one per case, in turn
        (e if k % 2 == 0 else w)[k % n] = SPECIALS[(k // 2) % len(SPECIALS)]
    return e, w


def _run_cases(n, cases):
    """Every case (ema offset, w offset, one_minus_decay, scale) in a slot of its own of two big buffers: sentinel, `off` elements, the n elements,
    sentinel.  One upload, one launch per case, one download; the whole ema buffer is compared, borders included."""
    from yolo_tf_amd import ops
    slot = (n + 16 + 3) // 4 * 4                                        # slots start on 16-byte boundaries; >= 4 sentinels on either side
    he = np.full(slot * len(cases), SENTINEL, np.float32)
    hw = np.full(slot * len(cases), SENTINEL, np.float32)
    want = he.copy()
    for k, (oe, ow, omd, scale) in enumerate(cases):
        e, w = _inputs(n, scale, k)
        a, b = k * slot + 4 + oe, k * slot + 4 + ow
        he[a:a + n], hw[b:b + n] = e, w
        want[a:a + n] = ema_ref.update(e, w, np.float32(omd))
    de, dw = torch.from_numpy(he).cuda(), torch.from_numpy(hw).cuda()
    assert de.data_ptr() % 16 == 0 and dw.data_ptr() % 16 == 0
    for k, (oe, ow, omd, scale) in enumerate(cases):
        a, b = k * slot + 4 + oe, k * slot + 4 + ow
        ops.ema_update(de[a:a + n], dw[b:b + n], n, float(np.float32(omd)))
    got = de.cpu().numpy()
    assert torch.equal(dw.cpu().view(torch.int32), torch.from_numpy(hw).view(torch.int32)), 'w was written'
    if not _bits_equal_nan_by_position(got, want):
        for k, case in enumerate(cases):
            s = slice(k * slot, (k + 1) * slot)
            assert _bits_equal_nan_by_position(got[s], want[s]), 'n = %d, (ema offset, w offset, one_minus_decay, scale) = %r' % (n, case)
    # the arithmetic was exercised: some result is neither input
    moved = [k for k, c in enumerate(cases) if 0.0 < c[2] < 1.0]
    assert not moved or any(not np.array_equal(got[k * slot:(k + 1) * slot], he[k * slot:(k + 1) * slot]) for k in moved)


@pytest.mark.parametrize('n', SIZES)
def test_kernel_equals_the_specification_bit_for_bit(n):
    if n <= 65536 + 3:
        cases = [(oe, ow, omd, sc) for (oe, ow) in OFFSETS for omd in OMDS for sc in SCALES]
        assert len(cases) == 240
        _run_cases(n, cases)
    else:
        # 4 M elements: every pair of offsets, the decays and magnitudes taken in turn (each at least three times), four cases per buffer
        cases = [(oe, ow, OMDS[k % len(OMDS)], SCALES[k % len(SCALES)]) for k, (oe, ow) in enumerate(OFFSETS)]
        for i in range(0, len(cases), 4):
            _run_cases(n, cases[i:i + 4])


def _fixed_batch(B=2, size=96, classes=20):
    from yolo_tf_amd.utils import data
    images = torch.rand(B, size, size, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0)) * 255
    return images, data.synthetic_batch(B, classes, size // 32, size // 32, seed=1)


def _assert_shadows_follow(session, w0, history, shadows, ema_decay):
    want = ema_ref.run(w0.cpu().numpy(), [h.cpu().numpy() for h in history], ema_decay)
    e = session.engine
    for t, (got, ref) in enumerate(zip(shadows, want), 1):
        got = got.cpu().numpy()
        for name, (o, n) in e.param_offsets.items():
            assert np.array_equal(got[o:o + n].view(np.int32), ref[o:o + n].view(np.int32)), 'step %d: %s' % (t, name)
    for name, (o, n) in e.param_offsets.items():                      # ema_var: the same ranges, as views of the arena
        assert session.ema_var[name].data_ptr() == session.ema[o:o + n].data_ptr() and session.ema_var[name].numel() == n
    assert set(session.ema_var) == set(e.param_offsets)


RECURRENCE = [
    # optimizer, gradient_clip, ema_decay, steps, deterministic, environment
    pytest.param('adam', 0.0, 0.999, 5, True, {}, id='adam-fused-0.999'),
    pytest.param('adam', 0.0, 0.5, 9, True, {}, id='adam-fused-0.5-both-sides-of-the-switch'),       # (1 + t) / (10 + t) for t <= 7, 0.5 from t = 8
    pytest.param('momentum', 5.0, 0.999, 5, True, {}, id='momentum-clip5-unfused'),
    pytest.param('adam', 0.0, 0.5, 3, False, {'YOLO2_EARLY_ADAM': '1'}, id='adam-layerwise-early-return'),
]


@pytest.mark.parametrize('optimizer,clip,ema_decay,steps,deterministic,env', RECURRENCE)
def test_session_shadows_follow_the_recurrence(basedir, monkeypatch, optimizer, clip, ema_decay, steps, deterministic, env):
    from yolo_tf_amd.session import TrainSession
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b, _ = make_builder('tiny', 20, 96, True, basedir)
    images, labels = _fixed_batch()
    sess = TrainSession(b, 2, dtype='f32', optimizer=optimizer, learning_rate=1e-3, gradient_clip=clip, seed=4, deterministic=deterministic,
                        ema_decay=ema_decay)
    assert sess.early_adam == bool(env)
    e = sess.engine
    assert sess.ema is not None and sess.ema.dtype == torch.float32 and sess.ema.numel() == e.n_params and sess.ema.data_ptr() != e.params.data_ptr()
    assert torch.equal(sess.ema, e.params)                             # [TF-sem] a shadow starts at its variable's initial value
    w0, history, shadows = e.params.clone(), [], []
    for _ in range(steps):
        sess.step(images, labels)
        history.append(e.params.clone())
        shadows.append(sess.ema.clone())
    torch.cuda.synchronize()
    assert sess.global_step == steps and not torch.equal(history[-1], w0)
    _assert_shadows_follow(sess, w0, history, shadows, ema_decay)
    assert not torch.equal(shadows[-1], history[-1]) and not torch.equal(shadows[-1], w0)


def test_the_average_does_not_disturb_training(basedir):
    from yolo_tf_amd.session import TrainSession
    b, _ = make_builder('tiny', 20, 96, True, basedir)
    images, labels = _fixed_batch()
    with_ema = TrainSession(b, 2, dtype='f32', optimizer='adam', learning_rate=1e-3, seed=4, deterministic=True, ema_decay=0.999)
    without = TrainSession(b, 2, dtype='f32', optimizer='adam', learning_rate=1e-3, seed=4, deterministic=True)
    assert without.ema is None and without.ema_var == {} and without.ema_decay == 0.0
    for _ in range(3):
        with_ema.step(images, labels)
        without.step(images, labels)
    torch.cuda.synchronize()
    assert torch.equal(with_ema.engine.params, without.engine.params) and torch.equal(with_ema.engine.state, without.engine.state)
    assert all(torch.equal(x, y) for x, y in zip(with_ema.optimizer.slots, without.optimizer.slots))
    assert with_ema.global_step == without.global_step == 3 and without.ema is None
    with pytest.raises(ValueError, match='ema_decay'):
        TrainSession(b, 2, dtype='f32', ema_decay=1.0)


@pytest.mark.parametrize('container', ['npz', 'tf'])
def test_checkpoint_round_trip(basedir, tmp_path, caplog, container):
    from yolo_tf_amd import checkpoint, tf_checkpoint
    from yolo_tf_amd.session import DetectSession, TrainSession
    C = checkpoint if container == 'npz' else tf_checkpoint
    b, _ = make_builder('tiny', 20, 96, True, basedir)
    images, labels = _fixed_batch()

    def fresh(ema_decay=0.9):
        return TrainSession(b, 2, dtype='f32', optimizer='adam', learning_rate=1e-3, seed=9, deterministic=True, ema_decay=ema_decay)
    a = fresh()
    for _ in range(3):
        a.step(images, labels)
    path = C.save(str(tmp_path / 'on'), a)
    c = fresh()
    assert C.restore(path, c) == 3
    assert torch.equal(c.ema, a.ema) and torch.equal(c.engine.params, a.engine.params) and not torch.equal(a.ema, a.engine.params)
    a.step(images, labels)
    c.step(images, labels)
    torch.cuda.synchronize()
    assert a.global_step == c.global_step == 4
    assert torch.equal(c.ema, a.ema) and torch.equal(c.engine.params, a.engine.params) and torch.equal(c.engine.state, a.engine.state)
    assert all(torch.equal(x, y) for x, y in zip(c.optimizer.slots, a.optimizer.slots))
    # written with the average off, restored into a session that keeps it: shadows = the restored parameters, one warning
    plain = fresh(ema_decay=None)
    assert plain.ema is None
    for _ in range(2):
        plain.step(images, labels)
    path_plain = C.save(str(tmp_path / 'off'), plain)
    d = fresh()
    caplog.clear()
    assert C.restore(path_plain, d) == 2
    assert torch.equal(d.engine.params, plain.engine.params) and torch.equal(d.ema, d.engine.params)
    assert len([r for r in caplog.records if 'moving averages' in r.getMessage()]) == 1
    # ... and a session without the average ignores the shadows of a file that has them
    plain2 = fresh(ema_decay=None)
    assert C.restore(path, plain2) == 3 and plain2.ema is None
    # the inference form
    bi, _ = make_builder('tiny', 20, 96, False, basedir)
    det = DetectSession(bi, 1, dtype='f32')
    saved = fresh()
    C.restore(path, saved)                                             # (a and c have moved on: the file's state again)
    raw, trainable = saved.engine.get_variables(), set(saved.engine.param_offsets)
    C.restore(path, engine=det.engine, ema=True)
    got = det.engine.get_variables()
    for name, v in raw.items():
        want = saved.ema_var[name].cpu().numpy().reshape(v.shape) if name in trainable else v
        assert np.array_equal(got[name].view(np.int32), want.view(np.int32)), name
    C.restore(path, engine=det.engine, ema=False)
    got = det.engine.get_variables()
    assert all(np.array_equal(got[name].view(np.int32), v.view(np.int32)) for name, v in raw.items())
    with pytest.raises(SystemExit) as exc:
        C.restore(path_plain, engine=det.engine, ema=True)
    assert str(path_plain) in str(exc.value) and '[mi355x] ema_decay' in str(exc.value)


def test_inference_uses_the_shadows(basedir, tmp_path):
    from yolo_tf_amd import checkpoint, ops
    from yolo_tf_amd.session import DetectSession, TrainSession
    b, _ = make_builder('tiny', 20, 96, True, basedir)
    images, labels = _fixed_batch()
    sess = TrainSession(b, 2, dtype='f32', optimizer='adam', learning_rate=1e-3, seed=9, deterministic=True, ema_decay=0.5)
    for _ in range(5):
        sess.step(images, labels)
    path = checkpoint.save(str(tmp_path), sess)
    raw = sess.engine.get_variables()
    shadow = dict(raw)
    for name in sess.engine.param_offsets:
        shadow[name] = sess.ema_var[name].cpu().numpy().reshape(raw[name].shape)
    bi, _ = make_builder('tiny', 20, 96, False, basedir)
    image = images[:1].clone()

    def logits(setup):
        det = DetectSession(bi, 1, dtype='f32')
        setup(det.engine)
        # The library's fixed-order launch rules for the four forwards: at 3 x 3 cells the default rules slice K over workgroups that meet in f32 atomics
        # (csrc/conv_igemm.hip), whose sums depend on arrival order -- two runs of ONE session then differ in the last bit, averages or not.
        # (five steps in, the moving statistics are still their initial values: the decoded boxes may overflow, so the logits are compared)
        with ops.deterministic_launches(True):
            det.run(image, check_numerics=False)
        torch.cuda.synchronize()
        out = det.engine.act[det.engine.output()][0].clone()
        assert torch.isfinite(out).all()
        return out
    from_ema = logits(lambda e: checkpoint.restore(path, engine=e, ema=True))
    from_raw = logits(lambda e: checkpoint.restore(path, engine=e, ema=False))
    set_ema = logits(lambda e: e.set_variables(shadow))
    set_raw = logits(lambda e: e.set_variables(raw))
    assert not torch.equal(from_ema, from_raw)
    assert torch.equal(from_ema, set_ema) and torch.equal(from_raw, set_raw)


# ---------------------------------------------------------------------------------------------------------------------
# data parallel: two processes on one GPU (the pattern of tests/test_network_gpu.py::test_data_parallel_step_two_processes_one_gpu)
# ---------------------------------------------------------------------------------------------------------------------
class _limit(object):
    """A time limit of its own around one GPU step of a worker: a step that hangs (a collective whose peer is gone) ends the process."""

    def __init__(self, seconds, what):
        import threading
        self.timer = threading.Timer(seconds, self._expire)
        self.timer.daemon = True
        self.what = what

    def _expire(self):
        import sys
        sys.stderr.write('time limit: %s\n' % self.what)
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()


def _ema_dp_worker(rank, world, port, outdir):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
    import torch.distributed as dist
    from yolo_tf_amd.parallel import init_distributed, sync_replicas
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    torch.cuda.set_device(0)
    with _limit(120, 'process group'):
        init_distributed(backend='gloo')                # both ranks share the one GPU of the test box: gloo carries the CUDA tensors
    rng = np.random.RandomState(100 + rank)             # different data per rank, same initial weights (same seed)
    images = torch.from_numpy(rng.uniform(0, 255, (2, 96, 96, 3)).astype(np.float32)).cuda()
    labels = data.synthetic_batch(2, 20, 3, 3, seed=200 + rank)
    out = {}
    b, _ = make_builder('tiny', 20, 96, True, os.path.join(outdir, 'base%d' % rank))
    for tag, shard in (('dp', False), ('shard', True)):
        with _limit(120, tag + ': session'):
            sess = TrainSession(b, 2, dtype='f32', optimizer='adam', learning_rate=1e-3, seed=3, world_size=world, bucket_mb=8.0, ema_decay=0.9,
                                shard_optimizer=shard)
            assert sess.shard_optimizer == shard and len(sess.reducer.buckets) >= 3 and sess.ema.numel() == sess.engine.n_params
            torch.cuda.synchronize()
        e = sess.engine
        if not shard:
            with _limit(120, 'sync_replicas'):
                if rank != 0:
                    sess.ema.fill_(7.0)                  # a rank whose shadows differ: rank 0's arrive with the parameters
                sync_replicas(sess)
                torch.cuda.synchronize()
                out['synced'] = sess.ema.cpu().numpy()
        w0 = e.params.clone()
        for step in range(3):
            with _limit(120, '%s: step %d' % (tag, step + 1)):
                sess.step(images, labels)
                torch.cuda.synchronize()
                out['%s/params%d' % (tag, step + 1)] = e.params.cpu().numpy()
        assert sess.global_step == 3
        out[tag + '/w0'], out[tag + '/ema'] = w0.cpu().numpy(), sess.ema.cpu().numpy()
    np.savez(os.path.join(outdir, 'rank%d.npz' % rank), **out)
    with _limit(120, 'shutdown'):
        dist.barrier()
        dist.destroy_process_group()


def test_data_parallel_ranks_keep_identical_shadows(tmp_path):
    """Every rank keeps the full average: after three steps (bucketed update, then the sharded update) both ranks' shadows are bitwise equal and equal the
    specification over rank 0's parameter history; sync_replicas carries rank 0's shadows to a rank that held others."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_ema_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(str(tmp_path / 'rank0.npz')), np.load(str(tmp_path / 'rank1.npz'))
    assert np.array_equal(r0['synced'].view(np.int32), r1['synced'].view(np.int32)) and not np.any(r1['synced'] == 7.0)
    assert np.array_equal(r0['synced'], r0['dp/w0'])
    for tag in ('dp', 'shard'):
        history = [r0['%s/params%d' % (tag, t)] for t in (1, 2, 3)]
        want = ema_ref.run(r0[tag + '/w0'], history, 0.9)[-1]
        assert np.array_equal(r0[tag + '/ema'].view(np.int32), r1[tag + '/ema'].view(np.int32)), tag
        assert np.array_equal(r0[tag + '/ema'].view(np.int32), want.view(np.int32)), tag
        assert not np.array_equal(r0[tag + '/ema'], history[-1]) and not np.array_equal(history[-1], r0[tag + '/w0'])
