"""Objectness-scaled distillation without a GPU: the specification (tests/distill_ref.py) against torch float64 autograd and its known answers, the
cases of tests/distill_cases.py and the proof that their bounds catch mistakes, the ``[distill]`` reader (yolo_tf_amd/distill.py), train.py's flags
and the refusals the builders alone decide."""
import argparse
import configparser
import os

import numpy as np
import pytest
import torch

import distill_cases as D
import distill_ref as S
import head_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(seed, shape=(2, 6, 3, 9)):
    rng = np.random.RandomState(seed)
    t = rng.randn(*shape) * 1.2
    return 0.5 * t + rng.randn(*shape) * 0.9, t


# ---------------------------------------------------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('class_term', S.CLASS_TERMS)
@pytest.mark.parametrize('T', [1.0, 2.5])
@pytest.mark.parametrize('scale', [True, False])
def test_hand_written_gradient_against_autograd(class_term, T, scale):
    s, t = _pair(1)
    opt = S.options(weight=0.7, objectness=1.5, coords=2.0, prob=0.5, class_term=class_term, temperature=T, scale_by_objectness=scale)
    st = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    o, c, p = S.terms(torch, st, torch.tensor(t, dtype=torch.float64), opt)
    S.total(opt, o, c, p).backward()
    auto = st.grad.numpy()
    g = S.gradient(s, t, opt)
    err = np.abs(g - auto).max() / np.abs(auto).max()
    print('%s T=%g scale=%s: hand-written against autograd, max |err| / max |g| = %.2e' % (class_term, T, scale, err))
    assert np.abs(auto).min() > 0 and err < 1e-12          # (every channel carries a gradient; float64 on both sides)
    obj, _ = S.loss(s, t, **opt)
    want = [float(v.detach()) for v in (o, c, p, S.total(opt, o, c, p))]                   # (NumPy and torch sum in different orders: float64 rounding apart)
    assert [obj[k] for k in ('objectness', 'coords', 'prob', 'distill')] == pytest.approx(want, rel=1e-13)


@pytest.mark.parametrize('class_term', S.CLASS_TERMS)
def test_identical_heads_give_zeros(class_term):
    s, _ = _pair(2)
    obj, g = S.loss(s, s, class_term=class_term, temperature=2.5)
    assert all(v == 0.0 for v in obj.values()) and not g.any()


@pytest.mark.parametrize('class_term', S.CLASS_TERMS)
def test_one_class_has_no_class_term(class_term):
    s, t = _pair(3, (2, 4, 3, 6))
    obj, g = S.loss(s, t, class_term=class_term, temperature=2.5)
    assert obj['prob'] == 0.0 and not g[..., 5:].any()
    assert obj['objectness'] > 0 and obj['coords'] > 0 and g[..., :5].all()


def test_a_teacher_that_sees_nothing_leaves_the_objectness_term():
    s, t = _pair(4)
    t[..., 0] = -40.0
    obj, g = S.loss(s, t)
    sg = 1 / (1 + np.exp(-s[..., 0]))
    assert obj['objectness'] == pytest.approx((sg ** 2).mean(), rel=1e-12)                 # (sigmoid(-40) = 4e-18)
    assert obj['coords'] < 1e-15 and obj['prob'] < 1e-16 and np.abs(g[..., 1:]).max() < 1e-17 and np.abs(g[..., 0]).min() > 1e-6
    raw, g_raw = S.loss(s, t, scale_by_objectness=False)                                   # ... and without the scale they are back
    assert raw['coords'] > 0.1 and raw['prob'] > 0.01 and np.abs(g_raw[..., 1:]).min() > 0


def test_accumulate_models_the_second_rounding():
    d0 = H.inputs64(np.float32([1.0, -0.37, 3e-3]), 'bf16')
    g = np.float64([2.0 ** -10, 1e-4, -2e-6])
    assert np.array_equal(S.accumulate(d0, g, 'f32'), (d0.astype(np.float32) + g.astype(np.float32)).astype(np.float64))
    out = S.accumulate(d0, g, 'bf16')
    assert np.array_equal(out, H.inputs64(out, 'bf16')) and out[0] == 1.0                  # 1 + 2^-10 rounds back to 1 in bf16 (8 significand bits)
    assert S.accumulate_ratio(out, d0, g, 'bf16') <= 1.0 and S.accumulate_ratio(d0 + 1.5 * g, d0, g, 'f32') > 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the cases and their bounds
# ---------------------------------------------------------------------------------------------------------------------

def test_cases_are_what_they_claim():
    assert set(D.SPECS) == {'pad3x4', 'one', 'sq13', 'rect9x14', 'saturated'}
    for name in D.SPECS:
        c = D.case(name)
        assert c['s'].shape == c['t'].shape == (c['B'], c['ch'] * c['cw'], c['A'], 5 + c['C']) and c['ld_s'] >= c['D'] and c['ld_t'] >= c['D']
    c = D.case('pad3x4')
    assert (c['ld_s'], c['ld_t'], c['D']) == (136, 125, 125)
    c = D.case('sq13')
    lanes = c['B'] * c['ch'] * c['cw'] * 8
    assert c['B'] * c['ch'] * c['cw'] * c['A'] == 1690 and lanes > 256 and lanes % 256 != 0      # several workgroups, a ragged last one
    c = D.case('saturated')
    for k in range(5 + c['C']):        # every channel holds the four saturated pairings
        col_s, col_t = c['s'][..., k].ravel(), c['t'][..., k].ravel()
        assert {(30, 30), (30, -30), (-30, 30), (-30, -30)} <= set(zip(col_s.tolist(), col_t.tolist()))
    for pair in D.PAIRS:
        for options in D.OPTIONS:
            obj, g = D.reference('saturated', pair, options)
            assert np.isfinite(g).all() and all(np.isfinite(v) for v in obj.values())
    obj, g = D.reference('one', ('f32', 'f32'), 'kl_T2.5')
    assert obj['prob'] == 0.0 and not g[..., 5:].any()


def test_the_specification_meets_its_own_bounds():
    for name in D.SPECS:
        for pair in D.PAIRS:
            for options in D.OPTIONS:
                obj, g = D.reference(name, pair, options)
                assert D.worst_ratio(name, pair, options, obj, g) <= 1.0
                obj32 = {k: float(np.float32(v)) for k, v in obj.items()}                  # ... and so does anything within f32's rounding of it
                assert D.worst_ratio(name, pair, options, obj32, g.astype(np.float32)) <= 1.0


@pytest.mark.parametrize('mutation,options', [('no_scale', 'mse'), ('no_scale', 'kl_T2.5'), ('no_inv_T', 'kl_T2.5'), ('no_inv_T', 'mse_T2.5_raw'),
                                              ('sign_w', 'mse'), ('sign_w', 'kl_raw')])
def test_the_bounds_catch_mistakes(mutation, options):
    """The reference with the scale m dropped, with a missing 1 / T factor in the class gradient, or with a sign error in one channel leaves the bounds
    of the GPU tests on every case it can show on, in every dtype pair."""
    for name in D.SPECS:
        if mutation == 'no_inv_T' and D.SPECS[name][4] == 1:
            continue                   # (one class: no class gradient to be wrong)
        for pair in D.PAIRS:
            s, t = D.read64(name, pair)
            obj, g = S.loss(s, t, mutation=mutation, **D.OPTIONS[options])
            ratio = D.worst_ratio(name, pair, options, obj, g)
            print('%s on %s %s/%s %s: %.3g x the bound' % (mutation, name, pair[0], pair[1], options, ratio))
            assert ratio > 1.0, (mutation, name, pair)


# ---------------------------------------------------------------------------------------------------------------------
# the [distill] reader and train.py's flags
# ---------------------------------------------------------------------------------------------------------------------

def _config(text=None):
    c = configparser.ConfigParser()
    c.read_string('[config]\nmodel = yolo2\n' + ('' if text is None else '[distill]\n' + text))
    return c


def test_reader_defaults_and_an_absent_section_mean_off():
    from yolo_tf_amd import distill
    want = dict(teacher=(), teacher_ckpt='', teacher_ema=False, teacher_dtype='bf16', weight=1.0, objectness=1.0, coords=1.0, prob=1.0, class_term='mse',
                temperature=1.0, scale_by_objectness=True)
    for cfg in (None, _config(), _config('')):
        got = distill.options(cfg)
        assert got == want and not distill.enabled(got)
    assert list(distill.KEYS) == list(want)
    assert not distill.enabled(distill.options(_config('teacher = a.ini\nweight = 0')))
    assert distill.enabled(distill.options(_config('teacher = a.ini')))
    shipped = configparser.ConfigParser()
    shipped.read(os.path.join(ROOT, 'config.ini'))
    assert not shipped.has_section('distill')                                            # the shipped file names every key, as comment lines
    with open(os.path.join(ROOT, 'config.ini')) as f:
        text = f.read()
    tail = text[text.index('\n; [distill]'):]
    assert text.index('\n; [distill]') > text.index('\n[summary]')
    for key in distill.KEYS:
        assert '\n; %s = ' % key in tail, key


def test_reader_reads_each_key():
    from yolo_tf_amd import distill
    cfg = _config('teacher = config.ini config/yolo2/darknet-20.ini\nteacher_ckpt = ~/t/model.ckpt-7.npz\nteacher_ema = yes\nteacher_dtype = F32\nweight = 0.5\n'
                  'objectness = 2\ncoords = 0\nprob = 1e-1\nclass_term = KL\ntemperature = 2.5\nscale_by_objectness = off')
    got = distill.options(cfg)
    assert got == dict(teacher=('config.ini', 'config/yolo2/darknet-20.ini'), teacher_ckpt='~/t/model.ckpt-7.npz', teacher_ema=True, teacher_dtype='f32',
                       weight=0.5, objectness=2.0, coords=0.0, prob=0.1, class_term='kl', temperature=2.5, scale_by_objectness=False)
    assert distill.kernel_options(got) == dict(weight=0.5, objectness=2.0, coords=0.0, prob=0.1, class_term='kl', temperature=2.5, scale_by_objectness=False)
    over = distill.options(cfg, weight=3.0, class_term='mse', scale_by_objectness=True, teacher=['x.ini'], teacher_ema=None)      # an argument wins, None does not
    assert (over['weight'], over['class_term'], over['scale_by_objectness'], over['teacher'], over['teacher_ema']) == (3.0, 'mse', True, ('x.ini',), True)


@pytest.mark.parametrize('text,match', [
    ('temperature = 0', r"\[distill\] temperature = '0': the temperature is positive and finite"),
    ('temperature = -1', 'temperature'), ('temperature = inf', 'temperature'), ('temperature = nan', 'temperature'), ('temperature = hot', r'temperature = .hot.: a number'),
    ('weight = -1', r"\[distill\] weight = '-1': a weight is >= 0 and finite"), ('objectness = -0.5', 'objectness'), ('coords = nan', 'coords'), ('prob = inf', 'prob'),
    ('class_term = ce', r"class_term = 'ce': one of mse, kl"), ('teacher_dtype = int8', 'an int8 teacher is out of scope'), ('teacher_dtype = f16', 'one of bf16, f32'),
    ('teacher_ema = maybe', 'true or false'), ('scale_by_objectness = 2', 'true or false')])
def test_reader_refusals(text, match):
    from yolo_tf_amd import distill
    with pytest.raises(ValueError, match=match):
        distill.options(_config('teacher = a.ini\n' + text))
    key, value = [p.strip() for p in text.split('=')]
    with pytest.raises(ValueError, match=match):                                         # the same value as an argument
        distill.options(None, **{key: value})


def test_reader_refuses_an_unknown_key():
    from yolo_tf_amd import distill
    with pytest.raises(ValueError, match='has no key hint'):
        distill.options(None, hint=1.0)


def test_train_flags():
    import train
    from yolo_tf_amd import distill
    a = train.make_args([])
    assert all(v is None for v in distill.from_args(a).values()) and set(distill.from_args(a)) == set(distill.KEYS)
    assert train.distill_setting(a, None) is None and train.distill_setting(a, _config()) is None             # no section, no flag: off
    a = train.make_args(['--teacher', 'config.ini', 'config/yolo2/darknet-20.ini', '--teacher_ckpt', 'x.npz', '--teacher_ema', '--teacher_dtype', 'f32', '--distill_weight', '2',
                         '--distill_objectness', '0.5', '--distill_coords', '3', '--distill_prob', '4', '--distill_class_term', 'kl', '--distill_temperature', '2.5',
                         '--no_distill_scale_by_objectness'])
    got = train.distill_setting(a, _config('weight = 9\nteacher_ema = no'))
    assert got == dict(teacher=('config.ini', 'config/yolo2/darknet-20.ini'), teacher_ckpt='x.npz', teacher_ema=True, teacher_dtype='f32', weight=2.0, objectness=0.5,
                       coords=3.0, prob=4.0, class_term='kl', temperature=2.5, scale_by_objectness=False)
    assert train.distill_setting(train.make_args(['--distill_weight', '0']), _config('teacher = a.ini')) is None
    assert train.distill_setting(train.make_args(['--no_teacher_ema']), _config('teacher = a.ini\nteacher_ema = 1'))['teacher_ema'] is False
    with pytest.raises(SystemExit):
        train.make_args(['--distill_class_term', 'ce'])
    with pytest.raises(ValueError, match='int8 teacher is out of scope'):
        train.distill_setting(train.make_args(['--teacher', 'a.ini', '--teacher_dtype', 'int8']), None)
    v1 = configparser.ConfigParser()
    v1.read_string('[config]\nmodel = yolo\n')
    with pytest.raises(ValueError, match=r'distillation covers the YOLOv2 family'):
        train.distill_setting(train.make_args(['--teacher', 'a.ini']), v1)
    assert train.distill_setting(train.make_args([]), v1) is None                                               # ... and off it refuses nothing


def test_event_scalars():
    import tempfile
    from yolo_tf_amd.utils import events
    base = dict(total_loss=3.0, iou_best=0.1, iou_normal=0.2, coords=0.3, prob=0.4)
    with tempfile.TemporaryDirectory() as d:
        for sub, fetched in (('off', base), ('on', dict(base, distill=1.5, distill_objectness=0.5, distill_coords=0.25, distill_prob=0.75))):
            w = events.FileWriter(os.path.join(d, sub))
            w.add_training_summary(7, fetched)
            w.close()
        tags = {}
        for sub in ('off', 'on'):
            (name,) = os.listdir(os.path.join(d, sub))
            tags[sub] = {}
            for ev in events.read_events(os.path.join(d, sub, name)):
                tags[sub].update(ev.get('scalars', {}))
    assert set(tags['off']) == {'total_loss'} | {'total_loss/objectives/' + k for k in ('iou_best', 'iou_normal', 'coords', 'prob')}
    assert set(tags['on']) - set(tags['off']) == {'total_loss/distill', 'total_loss/distill/objectness', 'total_loss/distill/coords', 'total_loss/distill/prob'}
    assert tags['on']['total_loss/distill'] == 1.5 and tags['on']['total_loss/distill/prob'] == 0.75


# ---------------------------------------------------------------------------------------------------------------------
# refusals of a pair of heads, decided by the builders alone
# ---------------------------------------------------------------------------------------------------------------------

class _Model(object):
    def __init__(self, anchors, classes, ch, cw):
        self.anchors, self.classes, self.cell_height, self.cell_width = np.asarray(anchors, np.float32), classes, ch, cw


def test_pair_refusals_on_plain_heads():
    from yolo_tf_amd import distill
    mk = lambda anchors=H.VOC_ANCHORS, C=20, grids={(416, 416): (13, 13)}, **kw: distill.head({wh: _Model(anchors, C, *g) for wh, g in grids.items()}, **kw)
    distill.refuse_pair(mk(batch=16), mk(batch=16))
    distill.refuse_pair(mk(batch=8), mk(batch=16))                                       # a larger teacher session is fine
    distill.refuse_pair(mk(grids={(416, 416): (13, 13)}), mk(grids={(416, 416): (13, 13), (320, 320): (10, 10)}))
    with pytest.raises(NotImplementedError, match='the student is a YOLO \\(v1\\) network'):
        distill.refuse_pair(mk(v1=True), mk())
    with pytest.raises(NotImplementedError, match='the teacher is a YOLO \\(v1\\) network'):
        distill.refuse_pair(mk(), mk(v1=True))
    with pytest.raises(NotImplementedError, match='int8 teacher is out of scope'):
        distill.refuse_pair(mk(), mk(int8=True))
    with pytest.raises(ValueError, match='the teacher has 3 anchors, the student 5'):
        distill.refuse_pair(mk(), mk(anchors=H.VOC_ANCHORS[:3]))
    with pytest.raises(ValueError, match='the teacher has 80 classes, the student 20'):
        distill.refuse_pair(mk(), mk(C=80))
    with pytest.raises(ValueError, match="the teacher's anchors differ"):
        distill.refuse_pair(mk(), mk(anchors=H.VOC_ANCHORS * 1.01))
    with pytest.raises(ValueError, match="at 416x416 the teacher's grid is 26x26, the student's 13x13"):
        distill.refuse_pair(mk(), mk(grids={(416, 416): (26, 26)}))
    with pytest.raises(ValueError, match='the student trains at 320x320, a size the teacher session was not built with'):
        distill.refuse_pair(mk(grids={(416, 416): (13, 13), (320, 320): (10, 10)}), mk())
    with pytest.raises(ValueError, match='the teacher session holds 8 images, the student 16'):
        distill.refuse_pair(mk(batch=16), mk(batch=8))


def test_pair_refusals_on_the_shipped_builders(tmp_path):
    """Darknet-19 and tiny share stride, anchors and classes; the 80-class teacher and the COCO anchors are refused."""
    from test_network_gpu import make_builder
    from yolo_tf_amd import distill
    heads = {}
    for inference, names in (('darknet', 20), ('tiny', 20), ('darknet', 80)):
        b, _ = make_builder(inference, names, 416, False, str(tmp_path / ('%s%d' % (inference, names))))
        heads[inference, names] = distill.head({(416, 416): b.model, (320, 320): b.trace(320, 320)[1]}, batch=4)
    distill.refuse_pair(heads['tiny', 20], heads['darknet', 20])
    assert heads['tiny', 20]['grids'] == heads['darknet', 20]['grids'] == {(416, 416): (13, 13), (320, 320): (10, 10)}
    with pytest.raises(ValueError, match='the teacher has 80 classes, the student 20'):
        distill.refuse_pair(heads['tiny', 20], heads['darknet', 80])
