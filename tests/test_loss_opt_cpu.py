"""The loss options without a GPU: the specification tests/loss_opt_ref.py against torch float64 autograd of a total loss written as one torch
expression; its identities; the conditions of the cases of tests/loss_opt_cases.py (asserted, not assumed); that the bounds of the GPU test are
attainable by float32 arithmetic and that they catch the mistakes a kernel could make; and the options' parsing and refusals.

One departure from "within half of the bounds with bf16-rounded stores": rounding a correct value to bf16 alone uses up to 0.95 of the bf16 bound
(2^-8 of 2^-8 + 1e-4; tests/test_box_loss_cpu.py met the same), so no store can sit within half of it.  As there, the float32 specification's
ARITHMETIC is held to half of the f32 bound on the inputs of both dtypes, and its bf16-STORED value to the bf16 bound itself."""
import argparse
import configparser
import ctypes

import numpy as np
import pytest
import torch

import box_loss_ref as BS
import head_cases as H
import loss_opt_cases as LC
import loss_opt_ref as S
from oracle import yolo2_ref as R

FIRST = [(n, LC.modes(n)[0]) for n in LC.CASES]
EVERY = [(n, m) for n in LC.CASES for m in LC.modes(n)]
SLOW_SCAN = ('dense32',)          # 5120 lanes x 1024 boxes: the restatement loops over a quarter of its lanes


def torch_total(c, mode, kw, aux):
    """The weighted total loss of a configuration as one torch float64 expression of the logits; the responsibility mask, the ignore mask and
    the IoU target come from the specification and are constants.  Returns (logits [B, cells, A, 5 + C] with .grad, total)."""
    B, cells, A, C = c['B'], c['ch'] * c['cw'], c['A'], c['C']
    T = lambda x: torch.tensor(np.asarray(x, np.float64))
    z = torch.tensor(H.inputs64(c['net'], mode).reshape(B, cells, A, 5 + C), requires_grad=True)
    mask, tprob, tcoords, tmin, tmax, tareas = [T(l) for l in c['labels']]
    mb, ign, iou_t = T(aux['mask_best']), torch.tensor(aux['ignored']), T(aux['iou'])
    cnt = float(B * cells * A)
    sg = torch.sigmoid(z[..., :3])
    wh = torch.exp(z[..., 3:5]) * T(c['anchors']).reshape(1, 1, A, 2)
    tgt = torch.where(mb != 0, iou_t, torch.zeros_like(mb)) if kw.get('rescore') else mb
    dist = (sg[..., 0] - tgt) ** 2
    obj = {'iou_best': (mb * dist).sum() / cnt, 'iou_normal': ((~ign) * (1 - mb) * dist).sum() / cnt}
    r = mb != 0
    if kw.get('box_loss', 'mse') == 'mse':
        coords = torch.cat([sg[..., 1:3], torch.sqrt(wh / T([c['cw'], c['ch']]))], -1)
        obj['coords'] = (mb[..., None] * (coords - tcoords) ** 2).sum() / cnt
    else:
        e = lambda x: x.expand(B, cells, A)[r]
        q = BS.score(torch, kw['box_loss'], sg[..., 1][r], sg[..., 2][r], wh[..., 0][r], wh[..., 1][r], e(tmin[..., 0]), e(tmin[..., 1]), e(tmax[..., 0]),
                     e(tmax[..., 1]), e(tareas))
        obj['coords'] = (mb[r] * (1 - q)).sum() / cnt
    logp = torch.log_softmax(z[..., 5:], -1)[r]
    t = tprob.expand(B, cells, A, C)[r]
    cls = kw.get('class_loss', 'mse')
    if cls == 'mse':
        term = ((torch.exp(logp) - t) ** 2).sum(-1)
    else:
        eps, gamma = kw.get('label_smoothing', 0.0), kw.get('focal_gamma', 2.0)
        tt = (1 - eps) * t + eps * t.sum(-1, keepdim=True) / C
        w = (1 - torch.exp(logp)) ** gamma if cls == 'focal' and gamma > 0 else 1.0
        term = -(tt * w * logp).sum(-1)
    obj['prob'] = (mb[r] * term).sum() / cnt
    return z, sum(H.HP[k] * obj[k] for k in R.OBJECTIVE_KEYS), obj


@pytest.mark.parametrize('name,mode', FIRST)
def test_specification_vs_autograd(name, mode):
    c = LC.case(name)
    for config, kw in LC.CONFIGS.items():
        ref = LC.reference(name, mode, config)
        z, total, obj = torch_total(c, mode, kw, ref['aux'])
        total.backward()
        want, got = z.grad.numpy().reshape(ref['dlogits'].shape), ref['dlogits']
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err <= 1e-9, (name, config, err)
        for k in R.OBJECTIVE_KEYS:
            assert abs(obj[k].item() - float(ref['obj'][k])) <= 1e-9 * abs(obj[k].item()) + 1e-300, (name, config, k)


@pytest.mark.parametrize('name,mode', EVERY)
def test_ignored_set_vs_triple_loop(name, mode):
    c = LC.case(name)
    m, labels = LC.decoded(name, mode)
    mask, _, _, tmin, tmax, tareas = labels
    B, cells, A, cw = c['B'], c['ch'] * c['cw'], c['A'], c['cw']
    M = np.zeros((B, cells, A))
    step = 4 if name in SLOW_SCAN else 1
    for b in range(B):
        js = np.flatnonzero(mask[b, :, 0])
        gx, gy = (js % cw).astype(np.float64), (js // cw).astype(np.float64)
        for i in range(0, cells, step):
            for a in range(A):
                x1, y1 = i % cw + m['offset_xy_min'][b, i, a]
                x2, y2 = i % cw + m['offset_xy_max'][b, i, a, 0], i // cw + m['offset_xy_max'][b, i, a, 1]
                y1 = i // cw + m['offset_xy_min'][b, i, a, 1]
                best = 0.0
                if len(js):
                    ix = np.maximum(np.minimum(x2, gx + tmax[b, js, 0, 0]) - np.maximum(x1, gx + tmin[b, js, 0, 0]), 0)
                    iy = np.maximum(np.minimum(y2, gy + tmax[b, js, 0, 1]) - np.maximum(y1, gy + tmin[b, js, 0, 1]), 0)
                    inter = ix * iy
                    best = float((inter / np.maximum(tareas[b, js, 0] + m['areas'][b, i, a] - inter, 1e-10)).max())
                M[b, i, a] = best
    ref = LC.max_gt_iou(name, mode)
    assert np.array_equal(M[:, ::step], ref[:, ::step])
    for config in ('ign3', 'ign6'):
        r = LC.reference(name, mode, config)
        want = (M > LC.CONFIGS[config]['ignore_thresh']) & (r['aux']['mask_best'] == 0)
        assert np.array_equal(want[:, ::step], r['aux']['ignored'][:, ::step])


@pytest.mark.parametrize('name,mode', EVERY)
def test_identities(name, mode):
    c = LC.case(name)
    net = H.inputs64(c['net'], mode)
    # all off is the oracle, exactly
    m = R.model_decode(net, c['C'], c['anchors'].astype(np.float64), training=True)
    obj0, aux0 = R.objectives(m, H.labels64(c['labels']))
    dl0 = R.loss_backward(m, H.labels64(c['labels']), aux0, H.HP, c['C'])
    off = LC.reference(name, mode, 'off')
    assert all(off['obj'][k] == obj0[k] for k in R.OBJECTIVE_KEYS) and np.array_equal(off['dlogits'], dl0)
    # focal with gamma 0 is ce
    for a, b in (('focal0', 'ce'), ('focal0_s', 'ce_s')):
        ra, rb = LC.reference(name, mode, a), LC.reference(name, mode, b)
        assert ra['obj'] == rb['obj'] and np.array_equal(ra['dlogits'], rb['dlogits'])
    # ce without smoothing on a one-hot row is -log p_target
    ce = LC.reference(name, mode, 'ce')
    mb, tprob = ce['aux']['mask_best'], c['labels'][1].astype(np.float64)
    logp = np.log(m['prob'])
    onehot = (tprob.sum(-1) == 1)
    want = np.where((mb != 0) & onehot, -np.take_along_axis(logp, np.broadcast_to(tprob.argmax(-1)[..., None], mb.shape + (1,)), -1)[..., 0], 0.0)
    z = m['inputs'][..., 5:]
    term, _ = S.class_term(z, np.broadcast_to(tprob, z.shape), 'ce', 0.0)
    sel = (mb != 0) & onehot
    assert np.allclose(term[sel], want[sel], rtol=1e-9, atol=1e-12)
    if onehot.all():
        assert abs(float(ce['obj']['prob']) - (mb * want).sum() / mb.size) <= 1e-9 * abs(float(ce['obj']['prob']))


@pytest.mark.parametrize('name,mode', EVERY)
def test_conditions_of_the_cases(name, mode):
    c = LC.case(name)
    M = LC.max_gt_iou(name, mode)
    mask = (c['labels'][0][..., 0] != 0)[..., None]
    for t in LC.THRESHOLDS:
        gap = float((np.abs(M - t) / t).min())
        assert gap > H.MARGIN, (name, mode, t, gap)
    ref = LC.reference(name, mode, 'ign6')
    for count, gap in H.margins(ref['aux']['iou'], c['labels'][0]):        # responsibility stays an unambiguous comparison in the new and the redrawn cases
        assert count == 1 or name in ('tie_all', 'tie_pair'), (name, count)
        assert gap > H.MARGIN, (name, mode, gap)
    if name in LC.IGNORE_CASES:
        for config in ('ign3', 'ign6'):
            r = LC.reference(name, mode, config)
            ign, t = r['aux']['ignored'], LC.CONFIGS[config]['ignore_thresh']
            assert (ign & mask).any(), (name, config, 'no ignored lane in an object cell')
            assert (ign & ~mask).any() or name not in LC.IGNORE_EMPTY_CELL, (name, config, 'no ignored lane in an empty cell')
            assert ((M > 0) & ~ign & (r['aux']['mask_best'] == 0)).any(), (name, config, 'no lane with M > 0 is kept')
            assert not (ign & (r['aux']['mask_best'] != 0)).any()


def test_special_cases_are_what_they_say():
    c = LC.case('multihot')
    rows = c['labels'][1][c['labels'][0][..., 0] != 0][:, 0]
    assert sorted(rows.sum(-1).tolist()).count(2.0) == c['B']                  # one two-bit row per image
    c = LC.case('onehot_sat')
    for mode in c['modes']:
        m, labels = LC.decoded('onehot_sat', mode)
        obj = labels[0][..., 0] != 0
        p_t = (m['prob'] * labels[1]).sum(-1)[obj]
        assert ((p_t > 1 - 1e-6) | (p_t < 1e-6)).all() and (p_t > 1 - 1e-6).any() and (p_t < 1e-6).any() and (p_t > 0).all() and (p_t < 1).all()
    c = LC.case('placed')
    for mode in c['modes']:
        r = LC.reference('placed', mode, 'ign6')
        M, iou, mask = r['aux']['M'], r['aux']['iou'], c['labels'][0][..., 0] != 0
        for b in range(c['B']):
            for (row, col, *_rest) in c['objs'][b]:
                cell = row * c['cw'] + col
                assert 0.85 < iou[b, cell, 0] < 0.95 and 0.65 < iou[b, cell, 1] < 0.75 and r['aux']['mask_best'][b, cell, 0] == 1
                assert 0.7 < M[b, cell - 1, 2] < 0.9 and not mask[b, cell - 1] and r['aux']['ignored'][b, cell - 1, 2] and r['aux']['ignored'][b, cell, 1]
    assert len(LC.case('dense19')['objs'][0]) == 361 and not LC.case('dense19')['objs'][1] and len(LC.case('dense32')['objs'][0]) == 1024
    assert any(not o for o in LC.case('g1x1')['objs']) and any(not o for o in LC.case('g2x3')['objs'])


def ratios(got_obj, got_dl, ref, mode):
    r = max(H.objective_ratio(got_obj[k], ref['obj'][k]) for k in R.OBJECTIVE_KEYS)
    return r, H.grad_ratio(got_dl, ref['dlogits'], mode)


@pytest.mark.parametrize('name,mode', EVERY)
def test_float32_specification_attains_the_bounds(name, mode):
    for config in LC.CONFIGS:
        ref, f32 = LC.reference(name, mode, config), LC.reference(name, mode, config, np.float32)
        assert np.array_equal(ref['aux']['ignored'], f32['aux']['ignored']) and np.array_equal(ref['aux']['mask_best'], f32['aux']['mask_best'])
        r_obj = max(H.objective_ratio(f32['obj'][k], ref['obj'][k]) for k in R.OBJECTIVE_KEYS)
        r_f32 = H.f32_ratio(f32['dlogits'], ref['dlogits'])
        r_store = H.grad_ratio(H.stored(f32['dlogits'], mode), ref['dlogits'], mode)
        assert r_obj <= 0.5, (name, mode, config, r_obj)
        if name not in LC.GRADIENT_CONDITION_EXEMPT:
            assert r_f32 <= 0.5 and r_store <= 1.0, (name, mode, config, r_f32, r_store)


MUTATION_PROOFS = {       # mutation -> (configuration, cases to look at)
    'other_image': ('ign6', ('placed', 'g2x3', 'dense19')),
    'no_own_cell': ('ign6', ('placed', 'g1x1')),
    'ignore_responsible': ('ign6', ('placed', 'g2x3')),
    'no_cell_xy': ('ign6', ('placed', 'g2x3')),
    'rescore_grad': ('rescore', ('placed', 'sq13_ld136')),
    'smooth_c_minus_1': ('ce_s', ('multihot', 'sq13_ld136')),
    'focal_half': ('focal2', ('sq13_ld136', 'multihot')),
    'smooth_mse': ('off', ('sq13_ld136',)),
}


@pytest.mark.parametrize('mutation', S.MUTATIONS)
def test_every_mutation_leaves_the_bounds_somewhere(mutation):
    config, names = MUTATION_PROOFS[mutation]
    worst = 0.0
    for name in names:
        for mode in LC.modes(name):
            ref, bad = LC.reference(name, mode, config), LC.reference(name, mode, config, mutation=mutation)
            worst = max(worst, *ratios(bad['obj'], H.stored(bad['dlogits'], mode), ref, mode))
    print('%s: worst |err| / bound %.3g' % (mutation, worst))
    assert worst > 1.0, mutation


# ---- option parsing ------------------------------------------------------------------------------------------------------------------

def _config(model='yolo2', **keys):
    cfg = configparser.ConfigParser()
    cfg.add_section('config')
    cfg.set('config', 'model', model)
    cfg.add_section('mi355x')
    for k, v in keys.items():
        cfg.set('mi355x', k, str(v))
    return cfg


def _args(**kw):
    base = dict(box_loss=None, class_loss=None, ignore_thresh=None, rescore=None, label_smoothing=None, focal_gamma=None)
    return argparse.Namespace(**dict(base, **kw))


def test_config_keys_and_command_line_overrides():
    import train
    from yolo_tf_amd.session import LOSS_OPTION_DEFAULTS, loss_options, loss_options_set
    assert loss_options(None) == LOSS_OPTION_DEFAULTS == loss_options(_config()) and loss_options_set(LOSS_OPTION_DEFAULTS) == []
    cfg = _config(class_loss='Focal', ignore_thresh=0.7, rescore='yes', label_smoothing=0.05, focal_gamma=1.5, box_loss='giou')
    want = dict(box_loss='giou', class_loss='focal', ignore_thresh=0.7, rescore=True, label_smoothing=0.05, focal_gamma=1.5)
    assert loss_options(cfg) == want == train.loss_setting(_args(), cfg)
    got = train.loss_setting(_args(class_loss='ce', ignore_thresh=0.0, rescore=False, label_smoothing=0.0, box_loss='mse'), cfg)       # the command line wins, towards off too
    assert got == dict(LOSS_OPTION_DEFAULTS, class_loss='ce', focal_gamma=1.5) and loss_options_set(got) == ['class_loss']
    assert train.describe_loss_options(LOSS_OPTION_DEFAULTS) is None
    assert train.describe_loss_options(want) == 'loss options: class_loss=focal, ignore_thresh=0.7, rescore=True, label_smoothing=0.05, focal_gamma=1.5'
    args = train.parse_args(['-c', 'config.ini', '--ignore_thresh', '0.6', '--rescore', '--class_loss', 'ce', '--label_smoothing', '0.1']) if hasattr(train, 'parse_args') else None
    if args is not None:
        assert (args.ignore_thresh, args.rescore, args.class_loss, args.label_smoothing, args.focal_gamma) == (0.6, True, 'ce', 0.1, None)
    import os
    text = open(os.path.join(os.path.dirname(os.path.abspath(train.__file__)), 'config.ini')).read()
    for key in ('; class_loss = ce', '; ignore_thresh = 0.6', '; rescore = true', '; label_smoothing = 0.1', '; focal_gamma = 2'):
        assert key in text, key


@pytest.mark.parametrize('bad,name', [(dict(class_loss='bce'), 'class_loss'), (dict(ignore_thresh=1.0), 'ignore_thresh'), (dict(ignore_thresh=-0.2), 'ignore_thresh'),
                                      (dict(ignore_thresh=float('nan')), 'ignore_thresh'), (dict(class_loss='focal', focal_gamma=0.5), 'focal_gamma'),
                                      (dict(class_loss='ce', label_smoothing=1.0), 'label_smoothing'), (dict(class_loss='ce', label_smoothing=-0.1), 'label_smoothing'),
                                      (dict(label_smoothing=0.1), 'label_smoothing'), (dict(box_loss='l1'), 'box_loss')])
def test_refusals_name_the_option(bad, name):
    import train
    from yolo_tf_amd import ops
    from yolo_tf_amd.session import loss_options
    with pytest.raises(ValueError, match=name):
        loss_options(None, **bad)
    with pytest.raises(ValueError, match=name):
        loss_options(_config(**bad))
    with pytest.raises(ValueError, match=name):
        ops.loss_options(**bad)
    with pytest.raises(ValueError, match=name):
        train.loss_setting(_args(**bad), _config())


def test_focal_gamma_is_read_with_focal_only():
    """A stray focal_gamma next to another class mode is accepted by the session, train.py, ops and the library alike."""
    import train
    from yolo_tf_amd import _lib, ops
    from yolo_tf_amd.session import loss_options
    assert loss_options(_config(focal_gamma=0.5))['class_loss'] == 'mse' and loss_options(None, class_loss='ce', focal_gamma=0.5)['focal_gamma'] == 0.5
    assert train.loss_setting(_args(focal_gamma=0.5), _config())['focal_gamma'] == 0.5
    assert ops.loss_options(focal_gamma=0.5) is None and ops.loss_options(class_loss='ce', focal_gamma=0.5).class_loss == 1
    one, hp = ctypes.c_void_p(64), (ctypes.c_float * 4)(1, 1, 1, 1)
    opt = _lib.LossOptions(28, 0, 1, 0, 0.0, 0.0, 0.5)
    with pytest.raises(_lib.HipKernelError, match='argument check failed: logits'):       # the options pass; the NULL logits are what is refused
        _lib.call('yolo2_loss_ex_partials', None, 136, one, one, one, one, one, one, one, hp, one, one, 2, 13, 13, 5, 20, 0, None, ctypes.byref(opt))


def test_yolo_v1_is_refused():
    import train
    for kw in (dict(class_loss='ce'), dict(ignore_thresh=0.6), dict(rescore=True)):
        with pytest.raises(ValueError, match='YOLO \\(v1\\)'):
            train.loss_setting(_args(**kw), _config(model='yolo'))
    assert train.loss_setting(_args(class_loss='mse'), _config(model='yolo', class_loss='ce'))['class_loss'] == 'mse'


def test_defaults_select_the_call_made_before_the_options_existed(monkeypatch):
    from yolo_tf_amd import _lib, ops
    names = []
    monkeypatch.setattr(ops, 'call', lambda name, *a: names.append(name))
    monkeypatch.setattr(ops, '_stream', lambda: None)
    x = torch.zeros(8)
    for kw, want in ((dict(), 'yolo2_loss'), (dict(box_loss='giou'), 'yolo2_loss_box'), (dict(class_loss='ce'), 'yolo2_loss_ex'), (dict(ignore_thresh=0.5), 'yolo2_loss_ex'),
                     (dict(rescore=True, box_loss='ciou'), 'yolo2_loss_ex'), (dict(focal_gamma=3.0), 'yolo2_loss')):
        del names[:]
        ops.loss(x, 8, x, [x] * 6, H.HPARAM, x, x, x, 1, 1, 1, 1, 3, **kw)
        ops.loss_partials(x, 8, x, [x] * 6, H.HPARAM, x, x, 1, 1, 1, 1, 3, **kw)
        assert names == [want, want + '_partials'], (kw, names)
    assert ops.loss_options() is None and ops.loss_options(box_loss='ciou') is None
    o = ops.loss_options(box_loss='ciou', class_loss='focal', ignore_thresh=0.6, rescore=True, label_smoothing=0.1, focal_gamma=1.0)
    assert (o.size, o.box_loss, o.class_loss, o.rescore) == (ctypes.sizeof(_lib.LossOptions), 4, 2, 1) and ctypes.sizeof(_lib.LossOptions) == 28
    assert _lib.CLASS_LOSSES == {'mse': 0, 'ce': 1, 'focal': 2}


def test_library_refuses_bad_options_before_any_device_work():
    from yolo_tf_amd import _lib
    one = ctypes.c_void_p(64)           # never dereferenced: the check comes first
    hp = (ctypes.c_float * 4)(1, 1, 1, 1)
    good = dict(size=28, box_loss=0, class_loss=0, rescore=0, ignore_thresh=0.0, label_smoothing=0.0, focal_gamma=2.0)
    bads = [dict(size=24), dict(size=32), dict(box_loss=5), dict(class_loss=3), dict(rescore=2), dict(ignore_thresh=1.0), dict(ignore_thresh=float('nan')),
            dict(label_smoothing=0.1), dict(class_loss=1, label_smoothing=1.0), dict(class_loss=2, focal_gamma=0.5), dict(class_loss=2, focal_gamma=float('inf'))]
    for bad in bads + [None]:
        ref = None if bad is None else ctypes.byref(_lib.LossOptions(**dict(good, **bad)))
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            _lib.call('yolo2_loss_ex', one, 136, one, one, one, one, one, one, one, hp, one, one, one, 2, 13, 13, 5, 20, 0, None, ref)
        with pytest.raises(_lib.HipKernelError, match='argument check failed'):
            _lib.call('yolo2_loss_ex_partials', one, 136, one, one, one, one, one, one, one, hp, one, one, 2, 13, 13, 5, 20, 0, None, ref)
