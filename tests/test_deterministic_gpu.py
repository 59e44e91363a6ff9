"""Deterministic training mode (TrainSession(deterministic=True)): same parameters, optimizer slots, BN state, global_step, image tensor and
labels => bitwise the same state after step(), whatever the buffer addresses.  The default path accumulates split filter gradients with f32 atomics in
an order that depends on the buffers' addresses (tests/test_network_gpu.py::test_tensorflow_checkpoint_and_event_file_round_trip), so two sessions built
one after the other in ONE process -- different addresses for everything -- are exactly the condition under which it differs."""
import os

import numpy as np
import pytest
import torch

from oracle import yolo2_ref as R

from test_network_gpu import HP, cosine, make_builder, rel, rel_l2, strip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def basedir():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        yield d


def _assert_sessions_equal(a, b, what):
    ea, eb = a.engine, b.engine
    assert ea.params.data_ptr() != eb.params.data_ptr() and ea.grads.data_ptr() != eb.grads.data_ptr()
    assert torch.equal(ea.params, eb.params), '%s: parameters' % what
    assert torch.equal(ea.state, eb.state), '%s: BN moving statistics' % what
    assert len(a.optimizer.slots) == len(b.optimizer.slots)
    for i, (x, y) in enumerate(zip(a.optimizer.slots, b.optimizer.slots)):
        assert torch.equal(x, y), '%s: optimizer slot %d' % (what, i)
    for name in ea.gvar:                                       # every parameter's gradient range (the gaps of the arena belong to nobody)
        assert torch.equal(ea.gvar[name], eb.gvar[name]), '%s: gradient of %s' % (what, name)
    assert a.global_step == b.global_step


CASES = [
    # inference, classes, construction size, sizes, dtype, batch, optimizer, gradient_clip
    pytest.param('darknet', 20, 416, None, 'bf16', 8, 'adam', 0.0, id='darknet20-416-bf16-b8'),       # split ranges on every non-13x13 layer
    pytest.param('tiny', 20, 160, None, 'f32', 4, 'adam', 0.0, id='tiny20-160-f32-b4'),
    pytest.param('darknet', 20, 416, [320, 416, 608], 'bf16', 8, 'adam', 0.0, id='darknet20-multiscale-bf16-b8'),
    pytest.param('darknet', 20, 416, None, 'bf16', 8, 'momentum', 5.0, id='darknet20-416-bf16-b8-clip5-momentum'),
]


@pytest.mark.parametrize('inference,classes,size,sizes,dtype,B,optimizer,clip', CASES)
def test_two_sessions_in_one_process_are_bitwise_equal(basedir, inference, classes, size, sizes, dtype, B, optimizer, clip):
    from yolo_tf_amd import ops
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    b, _ = make_builder(inference, classes, size, True, basedir)
    run_sizes = sizes or [size] * 3
    gen = torch.Generator(device='cuda').manual_seed(11)
    batches = [(torch.rand(B, s, s, 3, device='cuda', generator=gen) * 255, data.synthetic_batch(B, classes, s // 32, s // 32, seed=40 + i))
               for i, s in enumerate(run_sizes)]

    def fresh():
        return TrainSession(b, B, dtype=dtype, optimizer=optimizer, learning_rate=1e-3, gradient_clip=clip, seed=4, deterministic=True,
                            sizes=[(s, s) for s in sizes] if sizes else None)
    sess = [fresh(), fresh()]                                  # both alive: every buffer of the second lies somewhere else
    assert all(s.deterministic and s.engine.deterministic and s.engine._plan_grad_zeroing() == [] for s in sess)
    fetched = [[], []]
    for step, (images, labels) in enumerate(batches):
        for i, s in enumerate(sess):
            if sizes:
                s.set_size(run_sizes[step], run_sizes[step])
            s.step(images, labels)
            fetched[i].append(s.fetch())
        torch.cuda.synchronize()
        _assert_sessions_equal(sess[0], sess[1], 'after step %d' % (step + 1))
    assert fetched[0] == fetched[1], (fetched[0], fetched[1])
    assert all(np.isfinite(f['total_loss']) for f in fetched[0]) and torch.isfinite(sess[0].engine.params).all()
    assert ops._lib.query('yolo2_get_deterministic') == 0        # (on only for the duration of a deterministic engine's own sweeps)


def test_checkpoint_round_trip_continues_bit_for_bit(basedir, tmp_path):
    """tests/test_network_gpu.py::test_tensorflow_checkpoint_and_event_file_round_trip's continuation check at its original intent: a bound of zero."""
    from yolo_tf_amd import tf_checkpoint
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    b, _ = make_builder('tiny', 20, 96, True, basedir)
    images = torch.rand(2, 96, 96, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0)) * 255
    labels = data.synthetic_batch(2, 20, 3, 3, seed=1)

    def fresh():
        return TrainSession(b, 2, dtype='f32', optimizer='adam', learning_rate=1e-3, seed=9, deterministic=True)
    a = fresh()
    for _ in range(3):
        a.step(images, labels)
    prefix = tf_checkpoint.save(str(tmp_path), a)
    c = fresh()
    assert tf_checkpoint.restore(prefix, c) == 3
    assert torch.equal(c.engine.params, a.engine.params) and torch.equal(c.engine.state, a.engine.state)
    assert all(torch.equal(x, y) for x, y in zip(c.optimizer.slots, a.optimizer.slots))
    a.step(images, labels)
    c.step(images, labels)
    torch.cuda.synchronize()
    assert c.global_step == 4 and a.global_step == 4
    assert torch.equal(c.engine.params, a.engine.params) and torch.equal(c.engine.state, a.engine.state)
    assert all(torch.equal(x, y) for x, y in zip(c.optimizer.slots, a.optimizer.slots))


@pytest.mark.parametrize('inference,size,dtype,B', [('darknet', 416, 'bf16', 8), ('tiny', 160, 'f32', 4)])
def test_poisoned_filter_gradients_are_overwritten(basedir, inference, size, dtype, B):
    """Every convolution filter's gradient range holds NaN before forward_backward(): all gradients are finite afterwards and bit for bit those of the
    clean run -- nothing accumulates into the arena, nothing needed clearing."""
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    b, _ = make_builder(inference, 20, size, True, basedir)
    sess = TrainSession(b, B, dtype=dtype, optimizer='adam', learning_rate=1e-3, seed=2, deterministic=True)
    e = sess.engine
    images = torch.rand(B, size, size, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5)) * 255
    sess.upload_labels(data.synthetic_batch(B, 20, size // 32, size // 32, seed=6))
    sess.forward_backward(images)
    torch.cuda.synchronize()
    clean = {k: v.clone() for k, v in e.gvar.items()}
    filters = [op['weights'].name for op in e.graph.ops if op['kind'] == 'conv']
    assert len(filters) >= 9
    for name in filters:
        e.gvar[name].fill_(float('nan'))
    sess.forward_backward(images)
    torch.cuda.synchronize()
    for k, v in e.gvar.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, clean[k]), k


@pytest.mark.parametrize('inference,size,dtype,B', [('darknet', 160, 'f32', 2), ('tiny', 160, 'f32', 2), ('darknet', 224, 'f32', 1),
                                                    ('darknet', 224, 'bf16', 2), ('tiny', 160, 'bf16', 4)])
def test_deterministic_train_step_matches_oracle(basedir, inference, size, dtype, B):
    """Parity is not traded away: tests/test_network_gpu.py::test_train_step_matches_oracle's cases and bounds, with deterministic=True."""
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    classes = 20
    b, cfg = make_builder(inference, classes, size, True, basedir)
    sess = TrainSession(b, B, dtype=dtype, optimizer='adam', learning_rate=1e-3, seed=3, deterministic=True)
    scope = 'yolo2_' + inference
    params0 = strip(sess.engine.get_variables(), scope)
    rng = np.random.RandomState(0)
    for k in list(params0):
        if k.endswith('gamma'):
            params0[k] = (rng.rand(*params0[k].shape) + 0.5).astype(np.float32)
        if k.endswith(('beta', 'biases')):
            params0[k] = (rng.randn(*params0[k].shape) * 0.1).astype(np.float32)
    sess.engine.set_variables({scope + '/' + k: v for k, v in params0.items()})
    cells = size // 32
    images = rng.uniform(0, 255, (B, size, size, 3)).astype(np.float32)
    labels = data.synthetic_batch(B, classes, cells, cells, seed=7)
    sess.step(torch.from_numpy(images).cuda(), labels)
    got = sess.fetch()
    e = sess.engine
    logits = e.act[e.output()][0].float().cpu().numpy().reshape(B, cells, cells, -1)[..., :b.model.inputs.c]
    grads = strip(e.get_gradients(), scope)
    params1 = strip(e.get_variables(), scope)
    spec = R.SPECS[inference](classes, len(b.anchors))
    x = np.stack([R.per_image_standardization(i) for i in images]).astype(np.float32)
    f32 = dtype == 'f32'
    new_params, _, info = R.train_step(spec, params0, {}, x, labels, classes, b.anchors, HP, 1e-3, 0, quant=None if f32 else R.bf16_round)
    tol_out, tol_loss = (1e-4, 1e-4) if f32 else (0.2, 3e-2)
    r = rel(logits, info['net'])
    l2 = sorted(((rel_l2(grads[k], info['grads'][k]), k) for k in grads), reverse=True)
    cs = sorted((cosine(grads[k], info['grads'][k]), k) for k in grads)
    print('deterministic %s %d %s: logits rel %.2e, loss %.6f vs %.6f; worst grad rel-L2 %s; worst cosine %s'
          % (inference, size, dtype, r, got['total_loss'], info['loss'], ['%s %.2e' % (k, v) for v, k in l2[:3]], ['%s %.5f' % (k, v) for v, k in cs[:3]]))
    assert r <= tol_out, 'logits rel err %.3e' % r
    for k in R.OBJECTIVE_KEYS:
        assert abs(got[k] - info['objectives'][k]) <= (tol_loss if f32 else 0.3) * abs(info['objectives'][k]) + 1e-7, (k, got[k], info['objectives'][k])
    assert abs(got['total_loss'] - info['loss']) <= tol_loss * abs(info['loss'])
    if f32:
        assert l2[0][0] <= 2e-2, 'worst gradient rel-L2 err %.3e at %s' % l2[0]
        assert cs[0][0] >= 0.9995, 'worst gradient cosine %.5f at %s' % cs[0]
        for k in ('conv0/weights', 'conv/weights', 'conv/biases'):
            du_g, du_r = params1[k] - params0[k], new_params[k] - params0[k]
            assert np.mean(np.sign(du_g) == np.sign(du_r)) > 0.98, k
        for k in params0:
            if k.endswith(('moving_mean', 'moving_variance')):
                assert rel(params1[k], new_params[k]) <= 1e-4, k
    else:
        ratio = sorted((np.linalg.norm(grads[k].astype(np.float64)) / (np.linalg.norm(info['grads'][k].astype(np.float64)) + 1e-300), k) for k in grads)
        med = float(np.median([c for c, _ in cs]))
        assert med >= 0.5 and cs[0][0] >= 0.2, (med, cs[0])
        assert 0.5 <= ratio[0][0] and ratio[-1][0] <= 2.0, (ratio[0], ratio[-1])


def test_default_mode_is_unchanged_beside_a_deterministic_session(basedir):
    """A deterministic=False session built next to a deterministic one still zeroes exactly the ranges the host query names, launches the atomic plans
    (yolo2_debug_last_wgrad_plan after its backward: a split plan, not direct) and keeps its fused statistics; building and running the deterministic
    session leaves the process environment as it was."""
    from yolo_tf_amd import ops
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    B, size = 8, 416
    env_before = dict(os.environ)
    b, _ = make_builder('darknet', 20, size, True, basedir)
    det = TrainSession(b, B, dtype='bf16', optimizer='adam', learning_rate=1e-3, seed=4, deterministic=True)
    dflt = TrainSession(b, B, dtype='bf16', optimizer='adam', learning_rate=1e-3, seed=4)
    assert dict(os.environ) == env_before
    assert not dflt.deterministic and not dflt.engine.deterministic and dflt.engine.wgrad_ws is None
    e = dflt.engine
    assert e.fuse_bn_stats and e.fuse_first_wgrad and e.bn_bwd_fused and not det.engine.bn_bwd_fused and not det.engine.fuse_bn_stats
    # the zero ranges the default engine plans = the accumulating layers of the host query, merged as before
    expect = []
    for op in e.graph.ops:
        if op['kind'] == 'conv':
            x = op['x']
            if ops.conv2d_wgrad_accumulates(B, x.h, x.w, op['cin'], e.act[x][1], op['cout'], ops.pad8(op['cout']), op['ksize'], e.dtype):
                off, n = e.param_offsets[op['weights'].name]
                expect.append((off, off + (n + 3) // 4 * 4))
    # ... merged exactly as before: touching ranges joined, gaps of up to 2^20 floats bridged (one launch less each)
    merged = []
    for a, c in sorted(expect):
        if merged and a - merged[-1][1] <= (1 << 20):
            merged[-1] = (merged[-1][0], max(merged[-1][1], c))
        else:
            merged.append((a, c))
    ranges = e._plan_grad_zeroing()
    assert expect and ranges == merged, (ranges, merged)
    assert sum(hi - lo for lo, hi in ranges) < e.n_params // 2                      # (the 13x13 3x3 layers, most of the arena, store and are not cleared)
    assert det.engine._plan_grad_zeroing() == []
    images = torch.rand(B, size, size, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) * 255
    labels = data.synthetic_batch(B, 20, size // 32, size // 32, seed=2)
    det.step(images, labels)
    dflt.step(images, labels)
    plan = ops.last_wgrad_plan()                   # the default session's last filter gradient: conv0, fused with its BN backward (no plan of its own), so conv1's
    det.step(images, labels)
    assert ops._lib.query('yolo2_get_deterministic') == 0      # the library's per-thread switch is on only inside a deterministic engine's sweeps
    torch.cuda.synchronize()
    assert (plan['pair'], plan['BC'], plan['BN'], plan['waves'], plan['direct']) == (9, 32, 64, 12, 0), plan      # conv1's atomic plan (conv_wgrad_c32.hip)
    assert dict(os.environ) == env_before
    assert np.isfinite(det.fetch()['total_loss']) and np.isfinite(dflt.fetch()['total_loss'])


def test_fixed_order_clip_matches_the_atomic_form_and_repeats_bitwise():
    """yolo2_clip_by_norm_fixed against yolo2_clip_by_norm on the same gradients (both sum squares in f64: they agree to f32 rounding of the scale), with a
    NaN-filled workspace (nothing needs clearing), segments of very different sizes, some clipped and some not; two calls at different addresses are bitwise
    equal."""
    from yolo_tf_amd import ops
    sizes = [3, 1024, 1, 70001, 9 * 512 * 1024, 425, 64 * 256 + 7]              # segment = the run between two offsets, whatever its length
    offs = np.concatenate([[0], np.cumsum(sizes)])
    seg = torch.tensor(offs, dtype=torch.int64, device='cuda')
    g0 = torch.randn(int(offs[-1]), device='cuda', generator=torch.Generator(device='cuda').manual_seed(3))
    g0[offs[1]:offs[2]] *= 1e-3                                      # a tensor below the clip norm: left alone
    nseg, clip = len(sizes), 5.0
    ref = g0.clone()
    ops.clip_by_norm(ref, seg, nseg, clip, torch.zeros(nseg, dtype=torch.float64, device='cuda'))
    outs = []
    for _ in range(2):
        g = g0.clone()
        ws = torch.full((ops.workspace_bytes('clip_fixed', nseg) // 8,), float('nan'), dtype=torch.float64, device='cuda')
        ops.clip_by_norm_fixed(g, seg, nseg, clip, ws)
        outs.append((g, ws))
    torch.cuda.synchronize()
    assert outs[0][0].data_ptr() != outs[1][0].data_ptr() and torch.equal(outs[0][0], outs[1][0])
    assert torch.isfinite(outs[0][0]).all() and torch.equal(outs[0][0][offs[1]:offs[2]], g0[offs[1]:offs[2]])
    # f64 sums on both sides: the norms agree to ~1e-15, the f32 scale factor to one rounding -> elements to 2^-23 relative (bound: 2 ulp)
    assert float(((outs[0][0] - ref).abs() - 2.4e-7 * ref.abs()).max()) <= 0.0
    for i in range(nseg):                                             # every segment's norm is min(its norm, clip)
        nrm = float(outs[0][0][offs[i]:offs[i + 1]].double().norm())
        want = min(float(g0[offs[i]:offs[i + 1]].double().norm()), clip)
        assert abs(nrm - want) <= 1e-6 * want, (i, nrm, want)
