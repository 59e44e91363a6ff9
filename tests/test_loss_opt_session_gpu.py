"""`TrainSession(class_loss=..., ignore_thresh=..., rescore=..., label_smoothing=..., focal_gamma=...)` and the `[mi355x]` keys of the same names:
the session's loss call with the options is the kernel tests/test_loss_opt_gpu.py checks, on the session's own logits; with the keys absent it is the
call made before the options existed.  Deterministic and multi-scale training run with the options on."""
import numpy as np
import pytest
import torch

import head_cases as H
import loss_opt_ref as S
from oracle import yolo2_ref as R
from test_box_loss_session_gpu import B, SIZE, _batch, _direct, _forward_backward, basedir      # noqa: F401 (basedir is a fixture)
from test_network_gpu import make_builder

pytestmark = pytest.mark.gpu
ALL = dict(box_loss='ciou', class_loss='focal', ignore_thresh=0.6, rescore=True, label_smoothing=0.1, focal_gamma=2.0)


@pytest.fixture
def entries(monkeypatch):
    """The names of the library entries ops calls, in order."""
    from yolo_tf_amd import ops
    names = []
    real = ops.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(ops, 'call', recording)
    return names


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_session_with_all_options(basedir, entries, dtype):      # noqa: F811
    from yolo_tf_amd.session import TrainSession
    b, _ = make_builder('tiny', 20, SIZE, True, basedir)
    s = TrainSession(b, B, dtype=dtype, optimizer='adam', learning_rate=1e-3, seed=3, **ALL)
    assert s.loss_options == ALL
    logits, ld, dl, labels = _forward_backward(s)
    assert 'yolo2_loss_ex_partials' in entries and 'yolo2_loss_partials' not in entries and 'yolo2_loss_box_partials' not in entries
    bits = torch.int32 if dtype == 'f32' else torch.int16
    assert torch.equal(dl.view(bits), _direct(s, logits, ld, **ALL).view(bits))
    assert not torch.equal(dl.view(bits), _direct(s, logits, ld, box_loss='ciou').view(bits))
    got = s.fetch()
    m = s.model
    D = s.A * (5 + s.C)
    net = logits.reshape(-1)[:B * m.cells * ld].float().cpu().numpy().reshape(B, m.cell_height, m.cell_width, ld)[..., :D].astype(np.float64)
    hp = dict(zip(R.OBJECTIVE_KEYS, s.hparam))
    lab = [np.asarray(l, np.float32).reshape(B, m.cells, 1, -1) if i in (1, 2, 3, 4) else np.asarray(l, np.float32).reshape(B, m.cells, 1) for i, l in enumerate(labels)]
    obj, _, _ = S.loss(net, lab, m.anchors, hp, s.C, **ALL)
    total = sum(float(obj[k]) * hp[k] for k in R.OBJECTIVE_KEYS)
    print('session, all options, %s: %s (specification %s), total_loss %.6g (%.6g)' % (dtype, {k: got[k] for k in R.OBJECTIVE_KEYS}, obj, got['total_loss'], total))
    assert all(H.objective_ratio(got[k], obj[k]) <= 1.0 for k in R.OBJECTIVE_KEYS)
    assert H.objective_ratio(got['total_loss'], total) <= 1.0


def test_session_with_the_keys_absent_makes_the_old_call(basedir, entries):      # noqa: F811
    import ctypes
    from yolo_tf_amd import ops
    from yolo_tf_amd._lib import call, dtype_code, ptr
    from yolo_tf_amd.session import LOSS_OPTION_DEFAULTS, TrainSession
    b, _ = make_builder('tiny', 20, SIZE, True, basedir)
    s = TrainSession(b, B, dtype='bf16', optimizer='adam', learning_rate=1e-3, seed=3)
    assert s.loss_options == LOSS_OPTION_DEFAULTS
    logits, ld, dl, _ = _forward_backward(s)
    assert 'yolo2_loss_partials' in entries and not [n for n in entries if n.startswith('yolo2_loss_ex') or n.startswith('yolo2_loss_box')]
    m = s.model
    old = torch.full((B * m.cells * ld,), float('nan'), dtype=logits.dtype, device='cuda')
    ws = torch.full((ops.loss_ws_floats(B, m.cells, s.A),), float('nan'), dtype=torch.float32, device='cuda')
    call('yolo2_loss_partials', ptr(logits), ld, ptr(s.anchors), *[ptr(l) for l in s.labels], (ctypes.c_float * 4)(*s.hparam), ptr(old), ptr(ws),
         B, m.cell_height, m.cell_width, s.A, s.C, dtype_code(logits.dtype), ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(dl.view(torch.int16), old.view(torch.int16))


def test_config_keys_and_constructor_arguments_agree(basedir):      # noqa: F811
    from yolo_tf_amd.session import TrainSession
    b, cfg = make_builder('tiny', 20, SIZE, True, basedir)
    for k, v in (('class_loss', 'ce'), ('ignore_thresh', '0.6'), ('rescore', 'true'), ('label_smoothing', '0.1')):
        cfg.set('mi355x', k, v)
    kw = dict(class_loss='ce', ignore_thresh=0.6, rescore=True, label_smoothing=0.1)
    by_key = TrainSession(b, B, dtype='f32', seed=3, config=cfg)
    by_arg = TrainSession(b, B, dtype='f32', seed=3, **kw)
    assert by_key.loss_options == by_arg.loss_options and by_key.loss_options['class_loss'] == 'ce'
    off = TrainSession(b, B, dtype='f32', seed=3, config=cfg, class_loss='mse', ignore_thresh=0.0, rescore=False, label_smoothing=0.0)      # the arguments win
    assert off.loss_options['class_loss'] == 'mse' and not off.loss_options['rescore'] and off.loss_options['ignore_thresh'] == 0.0
    for s in (by_key, by_arg):
        logits, ld, dl, _ = _forward_backward(s)
        assert torch.equal(dl.view(torch.int32), _direct(s, logits, ld, **kw).view(torch.int32))
    for k in kw:
        cfg.remove_option('mi355x', k)
    with pytest.raises(ValueError, match='class_loss'):
        TrainSession(b, B, dtype='f32', class_loss='bce')


def _state(s):
    return [t.clone() for t in (s.engine.params, s.engine.gact[s.engine.output()][0])]


def test_two_deterministic_runs_with_all_options_repeat_bitwise(basedir):      # noqa: F811
    from yolo_tf_amd.session import TrainSession
    images, labels = _batch()
    runs = []
    for _ in range(2):
        b, _cfg = make_builder('tiny', 20, SIZE, True, basedir)
        s = TrainSession(b, B, dtype='bf16', optimizer='adam', learning_rate=1e-3, seed=3, deterministic=True, **ALL)
        for _step in range(2):
            s.step(images, labels)
        torch.cuda.synchronize()
        runs.append(_state(s) + [torch.tensor([s.fetch()[k] for k in R.OBJECTIVE_KEYS])])
    for a, c in zip(*runs):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32), c.view(torch.int16) if c.dtype == torch.bfloat16 else c.view(torch.int32))


def test_multi_scale_changes_grid_with_the_options_on(basedir, entries):      # noqa: F811
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    b, _ = make_builder('tiny', 20, SIZE, True, basedir)
    s = TrainSession(b, B, dtype='f32', optimizer='adam', learning_rate=1e-3, seed=3, sizes=[(64, 64), (96, 96)], **ALL)
    grids = []
    for w in (64, 96, 64):
        s.set_size(w, w)
        images = torch.rand(B, w, w, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(w)) * 255
        s.step(images, data.synthetic_batch(B, 20, w // 32, w // 32, seed=w))
        got = s.fetch()
        assert np.isfinite(got['total_loss'])
        grids.append((s.model.cell_height, s.model.cell_width))
    assert grids == [(2, 2), (3, 3), (2, 2)] and entries.count('yolo2_loss_ex_partials') == 3


def test_yolo_v1_is_refused_before_device_work(basedir):      # noqa: F811
    import os
    from test_network_gpu import ROOT
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
    for kw, text in ((dict(class_loss='ce'), 'class_loss = ce covers the YOLOv2 family'), (dict(ignore_thresh=0.6), 'ignore_thresh = 0.6 covers the YOLOv2 family'),
                     (dict(rescore=True), 'rescore = True covers the YOLOv2 family')):
        with pytest.raises(NotImplementedError, match=text):
            TrainSession(b, B, dtype='f32', **kw)
    assert torch.cuda.memory_allocated() == before
