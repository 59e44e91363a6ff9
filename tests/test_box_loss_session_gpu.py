"""`TrainSession(box_loss=...)` / `[mi355x] box_loss`: the session's loss call with the option is the kernel tests/test_box_loss_gpu.py checks, on
the session's own logits; without the option it is the call made before the option existed."""
import os
import tempfile

import numpy as np
import pytest
import torch

import box_loss_ref as S
import head_cases as H
from oracle import yolo2_ref as R
from test_network_gpu import ROOT, make_builder

pytestmark = pytest.mark.gpu
SIZE, B = 64, 2          # the smallest input the suite trains tiny-20 at: a 2x2 grid


@pytest.fixture(scope='module')
def basedir():
    with tempfile.TemporaryDirectory() as d:
        yield d


def _batch():
    from yolo_tf_amd.utils import data
    images = torch.rand(B, SIZE, SIZE, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0)) * 255
    return images, data.synthetic_batch(B, 20, SIZE // 32, SIZE // 32, seed=1)


def _forward_backward(session):
    """One forward_backward; returns (logits tensor, ld, the session's dlogits as a clone)."""
    images, labels = _batch()
    session.upload_labels(labels)
    session.forward_backward(images)
    torch.cuda.synchronize()
    e = session.engine
    out = e.output()
    (logits, ld), (dlogits, _) = e.act[out], e.gact[out]
    n = B * session.model.cells * ld
    return logits, ld, dlogits.reshape(-1)[:n].clone(), labels


def _direct(session, logits, ld, **kw):
    from yolo_tf_amd import ops
    m = session.model
    n = B * m.cells * ld
    dl = torch.full((n,), float('nan'), dtype=logits.dtype, device='cuda')
    ws = torch.full((ops.loss_ws_floats(B, m.cells, session.A),), float('nan'), dtype=torch.float32, device='cuda')
    ops.loss_partials(logits, ld, session.anchors, session.labels, session.hparam, dl, ws, B, m.cell_height, m.cell_width, session.A, session.C, **kw)
    torch.cuda.synchronize()
    return dl


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_session_with_ciou(basedir, dtype):
    from yolo_tf_amd.session import TrainSession
    b, _ = make_builder('tiny', 20, SIZE, True, basedir)
    s = TrainSession(b, B, dtype=dtype, optimizer='adam', learning_rate=1e-3, seed=3, box_loss='ciou')
    assert s.box_loss == 'ciou'
    logits, ld, dl, labels = _forward_backward(s)
    bits = torch.int32 if dtype == 'f32' else torch.int16
    assert torch.equal(dl.view(bits), _direct(s, logits, ld, box_loss='ciou').view(bits))
    assert not torch.equal(dl.view(bits), _direct(s, logits, ld).view(bits))                  # (and it is not the squared error's gradient)
    got = s.fetch()
    m = s.model
    D = s.A * (5 + s.C)
    net = logits.reshape(-1)[:B * m.cells * ld].float().cpu().numpy().reshape(B, m.cell_height, m.cell_width, ld)[..., :D].astype(np.float64)
    hp = dict(zip(R.OBJECTIVE_KEYS, s.hparam))
    lab = [np.asarray(l, np.float32).reshape(B, m.cells, 1, -1) if i in (1, 2, 3, 4) else np.asarray(l, np.float32).reshape(B, m.cells, 1) for i, l in enumerate(labels)]
    obj, _, _ = S.loss(net, lab, m.anchors, hp, s.C, 'ciou')
    total = sum(float(obj[k]) * hp[k] for k in R.OBJECTIVE_KEYS)
    print('session ciou %s: coords %.6g (specification %.6g), total_loss %.6g (%.6g)' % (dtype, got['coords'], obj['coords'], got['total_loss'], total))
    assert H.objective_ratio(got['coords'], obj['coords']) <= 1.0
    assert H.objective_ratio(got['total_loss'], total) <= 1.0


def test_session_without_the_option_makes_the_old_call(basedir):
    from yolo_tf_amd import ops
    from yolo_tf_amd.session import TrainSession
    b, _ = make_builder('tiny', 20, SIZE, True, basedir)
    s = TrainSession(b, B, dtype='bf16', optimizer='adam', learning_rate=1e-3, seed=3)
    assert s.box_loss == 'mse'
    logits, ld, dl, _ = _forward_backward(s)
    # the old entry, called directly
    from yolo_tf_amd._lib import call, dtype_code, ptr
    import ctypes
    m = s.model
    n = B * m.cells * ld
    old = torch.full((n,), float('nan'), dtype=logits.dtype, device='cuda')
    ws = torch.full((ops.loss_ws_floats(B, m.cells, s.A),), float('nan'), dtype=torch.float32, device='cuda')
    call('yolo2_loss_partials', ptr(logits), ld, ptr(s.anchors), *[ptr(l) for l in s.labels], (ctypes.c_float * 4)(*s.hparam), ptr(old), ptr(ws),
         B, m.cell_height, m.cell_width, s.A, s.C, dtype_code(logits.dtype), ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(dl.view(torch.int16), old.view(torch.int16))


def test_config_key_and_constructor_argument_agree(basedir):
    from yolo_tf_amd.session import TrainSession
    b, cfg = make_builder('tiny', 20, SIZE, True, basedir)
    cfg.set('mi355x', 'box_loss', 'giou')
    by_key = TrainSession(b, B, dtype='f32', seed=3, config=cfg)
    by_arg = TrainSession(b, B, dtype='f32', seed=3, box_loss='giou')
    assert by_key.box_loss == by_arg.box_loss == 'giou'
    assert TrainSession(b, B, dtype='f32', seed=3, config=cfg, box_loss='mse').box_loss == 'mse'          # the argument wins
    for s in (by_key, by_arg):          # (each on its own logits: two sessions' forwards sum in arrival order and need not agree to the bit)
        logits, ld, dl, _ = _forward_backward(s)
        assert torch.equal(dl.view(torch.int32), _direct(s, logits, ld, box_loss='giou').view(torch.int32))
    cfg.remove_option('mi355x', 'box_loss')
    with pytest.raises(ValueError, match='box_loss'):
        TrainSession(b, B, dtype='f32', box_loss='l1')


def test_yolo_v1_is_refused_before_device_work(basedir):
    from yolo_tf_amd import utils
    from yolo_tf_amd.model import yolo
    from yolo_tf_amd.session import TrainSession
    cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo', 'tiny-20.ini')], basedir)
    cfg.set('cache', 'names', os.path.join(ROOT, cfg.get('cache', 'names')))
    utils.ensure_names(cfg)
    b = yolo.Builder(None, cfg)
    b(None, training=True)
    b.create_objectives()
    before = torch.cuda.memory_allocated()
    with pytest.raises(NotImplementedError, match='box_loss = giou covers the YOLOv2 family'):
        TrainSession(b, B, dtype='f32', box_loss='giou')
    assert torch.cuda.memory_allocated() == before              # no engine, no buffer
