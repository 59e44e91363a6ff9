"""`TrainSession(teacher=, distill=)`: off is the session as it was, bit for bit; on, the student's logit gradient is the loss's plus the specification's
distill gradient (tests/distill_ref.py) on the two sessions' own logits, `fetch()` reports the terms, steps stay bitwise reproducible, `set_size`
switches the teacher too, and a pair the kernel cannot compare is refused before any launch."""
import os
import tempfile

import numpy as np
import pytest
import torch

import distill_ref as S
import head_cases as H
from test_network_gpu import ROOT, make_builder

pytestmark = pytest.mark.gpu
SIZE, B = 64, 2          # the smallest input the suite trains tiny-20 at: a 2x2 grid
OPT = dict(weight=0.7, objectness=1.5, coords=2.0, prob=0.5, class_term='kl', temperature=2.5)
BITS = {'f32': torch.int32, 'bf16': torch.int16}


@pytest.fixture(scope='module')
def basedir():
    with tempfile.TemporaryDirectory() as d:
        yield d


def _batch(size=SIZE, seed=0):
    from yolo_tf_amd.utils import data
    images = torch.rand(B, size, size, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(seed)) * 255
    return images, data.synthetic_batch(B, 20, size // 32, size // 32, seed=seed + 1)


def _teacher(basedir, dtype='bf16', batch=B, names=20, sizes=None, size=SIZE):
    from yolo_tf_amd.session import DetectSession
    b, _ = make_builder('tiny', names, size, False, basedir)
    return DetectSession(b, batch, dtype=dtype, seed=11, sizes=sizes)          # another seed than the students': other weights


def _student(basedir, dtype='bf16', **kw):
    from yolo_tf_amd.session import TrainSession
    b, _ = make_builder('tiny', 20, SIZE, True, basedir)
    return TrainSession(b, B, dtype=dtype, optimizer='adam', learning_rate=1e-3, seed=3, deterministic=True, **kw)


def _state(s):
    e = s.engine
    return [e.params.clone(), e.state.clone()] + [slot.clone() for slot in s.optimizer.slots]


def _steps(s, n=2):
    for i in range(n):
        images, labels = _batch(seed=10 * i)
        s.step(images, labels)
    torch.cuda.synchronize()
    return _state(s), s.fetch()


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _rows(t, ld, cells, D):
    return t.reshape(-1)[:B * cells * ld].float().cpu().numpy().reshape(B, cells, ld)[..., :D].astype(np.float64)


def test_off_is_the_session_as_it_was(basedir):
    def buffers(s):
        """Every device tensor the session or its engine holds, by attribute name: shape and dtype.  (The allocator's byte count is no yardstick: a
        cached block that is handed out again may be larger than what was asked for.)"""
        return {(o, k): (tuple(v.shape), v.dtype) for o, obj in (('session', s), ('engine', s.engine)) for k, v in vars(obj).items() if torch.is_tensor(v)}

    s = _student(basedir)
    held = buffers(s)
    plain, fetched = _steps(s)
    teacher = _teacher(basedir)
    for kw in (dict(teacher=None, distill=OPT), dict(teacher=teacher, distill=dict(OPT, weight=0.0))):
        s = _student(basedir, **kw)
        assert s.teacher is None and s.distill is None and not hasattr(s, 'distill_ws') and not hasattr(s, 'distill_dev')
        assert buffers(s) == held                          # not a buffer more than the session without the arguments
        state, got = _steps(s)
        assert _same(state, plain)
        assert got == fetched and 'distill' not in got


@pytest.mark.parametrize('dtype,teacher_dtype', [('f32', 'f32'), ('bf16', 'bf16'), ('bf16', 'f32')])
def test_gradient_and_scalars_against_the_specification(basedir, dtype, teacher_dtype):
    t = _teacher(basedir, teacher_dtype)
    twin, s = _student(basedir, dtype), _student(basedir, dtype, teacher=t, distill=OPT)
    assert s.teacher is t and s.distill == dict(S.DEFAULTS, **OPT)
    images, labels = _batch()
    out = {}
    for name, sess in (('twin', twin), ('distill', s)):
        sess.upload_labels(labels)
        sess.forward_backward(images)
        torch.cuda.synchronize()
        e = sess.engine
        (logits, ld), (dlogits, _) = e.act[e.output()], e.gact[e.output()]
        out[name] = (logits, ld, dlogits.reshape(-1)[:B * sess.model.cells * ld].clone())
    (l0, ld, d0), (l1, _, d1) = out['twin'], out['distill']
    m = s.model
    n = B * m.cells * ld
    assert torch.equal(l0.reshape(-1)[:n].view(BITS[dtype]), l1.reshape(-1)[:n].view(BITS[dtype]))          # deterministic twins: the same logits, so d0 is the loss's part
    D = s.A * (5 + s.C)
    shape = (B, m.cells, s.A, 5 + s.C)
    t_logits, t_ld = t.engine.act[t.engine.output()]
    assert t_logits.dtype == {'f32': torch.float32, 'bf16': torch.bfloat16}[teacher_dtype]
    obj, g = S.loss(_rows(l1, ld, m.cells, D).reshape(shape), _rows(t_logits, t_ld, m.cells, D).reshape(shape), **OPT)
    assert np.abs(g).min() > 0
    ratio = S.accumulate_ratio(_rows(d1, ld, m.cells, D), _rows(d0, ld, m.cells, D), g.reshape(B, m.cells, D), dtype)
    pad = d1.float().cpu().numpy().reshape(B, m.cells, ld)[..., D:]
    got, base = s.fetch(), twin.fetch()
    ratios = {k: H.objective_ratio(got['distill' + ('_' + k if k != 'distill' else '')], obj[k]) for k in ('objectness', 'coords', 'prob', 'distill')}
    print('session distill %s/%s: accumulated gradient worst |err| / bound = %.3f; scalars %s, |err| / (1e-04 |ref|) %s'
          % (dtype, teacher_dtype, ratio, {k: got[k] for k in got if k.startswith('distill')}, ratios))
    assert ratio <= 1.0
    assert not pad.any(), 'padding channels stay as the loss left them'
    assert max(ratios.values()) <= 1.0
    assert all(got[k] == base[k] for k in ('iou_best', 'iou_normal', 'coords', 'prob'))
    assert got['total_loss'] == base['total_loss'] + got['distill']


def test_two_deterministic_runs_are_bitwise_equal(basedir):
    runs = [_steps(_student(basedir, teacher=_teacher(basedir), distill=OPT)) for _ in range(2)]
    assert _same(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert np.isfinite(runs[0][1]['distill']) and runs[0][1]['distill'] > 0
    plain, _ = _steps(_student(basedir))
    assert not _same(runs[0][0], plain)                    # ... and the teacher did move the weights


def test_set_size_switches_the_teacher_too(basedir):
    from yolo_tf_amd.session import TrainSession
    from yolo_tf_amd.utils import data
    sizes = [(SIZE, SIZE), (96, 96)]
    t = _teacher(basedir, sizes=sizes)
    b, _ = make_builder('tiny', 20, SIZE, True, basedir)
    s = TrainSession(b, B, dtype='bf16', optimizer='adam', learning_rate=1e-3, seed=3, sizes=sizes, teacher=t, distill=OPT)
    assert s.size == t.size == (SIZE, SIZE)
    for size in (96, SIZE):
        s.set_size(size, size)
        assert s.size == t.size == (size, size) and (t.model.cell_height, t.model.cell_width) == (s.model.cell_height, s.model.cell_width) == (size // 32, size // 32)
        images, labels = _batch(size)
        s.step(images, labels)
        got = s.fetch()
        assert all(np.isfinite(got[k]) for k in ('total_loss', 'distill', 'distill_objectness', 'distill_coords', 'distill_prob')) and got['distill'] > 0
        assert t.engine.act[t.engine.output()][0].numel() >= B * (size // 32) ** 2 * s.A * (5 + s.C)


def test_a_larger_teacher_session_reads_the_students_batch(basedir):
    big, same = _teacher(basedir, batch=B + 1), _teacher(basedir)
    a, b = _student(basedir, teacher=big, distill=OPT), _student(basedir, teacher=same, distill=OPT)
    (sa, fa), (sb, fb) = _steps(a, 1), _steps(b, 1)
    assert _same(sa, sb) and fa == fb


def test_refusals_come_before_any_launch(basedir):
    from yolo_tf_amd import utils
    from yolo_tf_amd.model import yolo
    from yolo_tf_amd.session import TrainSession
    small, coco, one_size = _teacher(basedir, batch=1), _teacher(basedir, names=80), _teacher(basedir)
    int8 = _teacher(basedir)
    int8.dtype = 'int8'           # (what a session built with dtype='int8' and a calibration says of itself)
    b, _ = make_builder('tiny', 20, SIZE, True, basedir)
    cfg = utils.make_config([os.path.join(ROOT, 'config.ini'), os.path.join(ROOT, 'config', 'yolo', 'tiny-20.ini')], basedir)
    cfg.set('cache', 'names', os.path.join(ROOT, cfg.get('cache', 'names')))
    utils.ensure_names(cfg)
    v1 = yolo.Builder(None, cfg)
    v1(None, training=True)
    v1.create_objectives()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for builder, teacher, kw, exc, match in (
            (b, small, {}, ValueError, 'the teacher session holds 1 images, the student 2'),
            (b, coco, {}, ValueError, 'the teacher has 80 classes, the student 20'),
            (b, one_size, dict(sizes=[(SIZE, SIZE), (96, 96)]), ValueError, 'the student trains at 96x96, a size the teacher session was not built with'),
            (b, int8, {}, NotImplementedError, 'int8 teacher is out of scope'),
            (v1, one_size, {}, NotImplementedError, 'the student is a YOLO \\(v1\\) network'),
            (b, one_size, dict(distill=dict(temperature=0.0)), ValueError, 'temperature'),
            (b, one_size, dict(distill=dict(class_term='ce')), ValueError, 'class_term')):
        with pytest.raises(exc, match=match):
            TrainSession(builder, B, dtype='f32', teacher=teacher, **kw)
        assert torch.cuda.memory_allocated() == before, match          # no engine, no buffer
