"""The loss options on the device (csrc/head.hip loss_kernel<T, MODE, CLS, EXT>, csrc/loss_opts.h; entries yolo2_loss_ex and
yolo2_loss_ex_partials) in f32 and bf16 against the float64 specification tests/loss_opt_ref.py, on the cases and the option matrix of
tests/loss_opt_cases.py.  The cases' own conditions and the proof that these bounds catch wrong losses are in tests/test_loss_opt_cpu.py.

Bounds: objectives 1e-4 relative (head_cases.objective_ratio); the channels of dlogits an option concerns head_cases.grad_ratio; the ignored
set exactly the specification's; everything an option does not concern bit-equal to what yolo2_loss writes for the same inputs.  Every output
buffer and the workspace start out filled with NaN."""
import ctypes

import numpy as np
import pytest
import torch

import head_cases as H
import loss_opt_cases as LC
from oracle import yolo2_ref as R
from test_box_loss_gpu import BITS, same_bits
from test_head_gpu import TDTYPE, nans, upload
from test_kernels_gpu import dev, host, pad_channels

pytestmark = pytest.mark.gpu

THREE = [('sq13_ld136', 'f32'), ('sq13_ld136', 'bf16'), ('rect9x14', 'f32'), ('rect9x14', 'bf16'), ('b8_19x19', 'bf16')]
ALONE = ['ign6', 'rescore', 'ce_s', 'focal2']


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def options(ops, **kw):
    """The yolo2_loss_options of a configuration, unchecked (refusals are the library's to make)."""
    from yolo_tf_amd._lib import BOX_LOSSES, CLASS_LOSSES, LossOptions
    return LossOptions(kw.get('size', ctypes.sizeof(LossOptions)), BOX_LOSSES[kw.get('box_loss', 'mse')], CLASS_LOSSES.get(kw.get('class_loss', 'mse'), kw.get('class_loss')),
                       int(kw.get('rescore', 0)), kw.get('ignore_thresh', 0.0), kw.get('label_smoothing', 0.0), kw.get('focal_gamma', 2.0))


def run(ops, name, mode, kw, split=False, ws=None, dl=None, entry='ex'):
    """One launch on NaN-filled outputs (or on the buffers handed in, as they are).  entry 'ex': yolo2_loss_ex / yolo2_loss_ex_partials called
    directly with the options ``kw``; 'old': yolo2_loss / yolo2_loss_partials; 'box': yolo2_loss_box[_partials] with kw's box_loss; 'ops': the
    ops wrappers with ``kw``.  Returns (objectives, dlogits, ws, dl buffer)."""
    from yolo_tf_amd._lib import BOX_LOSSES, call, dtype_code, ptr
    c = LC.case(name)
    B, ch, cw, A, C, ld = c['B'], c['ch'], c['cw'], c['A'], c['C'], c['ld']
    cells = ch * cw
    logits = upload(pad_channels(c['net'], ld), mode)
    labels = [dev(l.reshape(B, cells, -1)) for l in c['labels']]
    anchors = dev(c['anchors'])
    n = B * cells * ld
    ws = nans(ops.loss_ws_floats(B, cells, A)) if ws is None else ws
    dl = nans(n, TDTYPE[mode]) if dl is None else dl
    objs = nans(4)
    hp = (ctypes.c_float * 4)(*H.HPARAM)
    args = [ptr(logits), ld, ptr(anchors)] + [ptr(l) for l in labels] + [hp]
    tail = [ptr(dl), ptr(ws), B, ch, cw, A, C, dtype_code(logits.dtype), ops._stream()]
    if entry == 'ops':
        if split:
            ops.loss_partials(logits, ld, anchors, labels, H.HPARAM, dl, ws, B, ch, cw, A, C, **kw)
        else:
            ops.loss(logits, ld, anchors, labels, H.HPARAM, objs, dl, ws, B, ch, cw, A, C, **kw)
    else:
        sym = {'ex': 'yolo2_loss_ex', 'old': 'yolo2_loss', 'box': 'yolo2_loss_box'}[entry]
        opt = options(ops, **kw)
        last = {'ex': [ctypes.byref(opt)], 'old': [], 'box': [BOX_LOSSES[kw.get('box_loss', 'mse')]]}[entry]
        if split:
            call(sym + '_partials', *(args + tail + last))
        else:
            call(sym, *(args + [ptr(objs)] + tail + last))
    if split:
        ops.loss_objectives(ws, objs, B, ch, cw, A)
    torch.cuda.synchronize()
    return objs, dl[:n].clone(), ws, dl


@pytest.fixture(scope='module')
def base(ops):
    """What yolo2_loss (or yolo2_loss_box) writes for a case and dtype, once per module."""
    cache = {}

    def get(name, mode, box_loss='mse'):
        if (name, mode, box_loss) not in cache:
            objs, dl, _, _ = run(ops, name, mode, dict(box_loss=box_loss), entry='old' if box_loss == 'mse' else 'box')
            cache[(name, mode, box_loss)] = (host(objs), host(dl))
        return cache[(name, mode, box_loss)]
    return get


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize('name,mode,config', LC.ALL)
def test_kernel_vs_specification(ops, base, name, mode, config):
    c, ref, kw = LC.case(name), LC.reference(name, mode, config), LC.CONFIGS[config]
    objs, dl, _, _ = run(ops, name, mode, kw)
    got, d = host(objs), host(dl).reshape(c['B'], c['ch'], c['cw'], c['ld'])
    what = 'loss options %s %s %s' % (name, mode, config)
    assert np.all(np.isfinite(got)) and not np.isnan(d).any(), what
    assert np.all(d[..., c['D']:] == 0), 'padding channels of dlogits'
    ratios = [H.objective_ratio(got[i], ref['obj'][k]) for i, k in enumerate(R.OBJECTIVE_KEYS)]
    obj_idx, chans = LC.concerned(config)
    grads = {}
    for which in chans:
        g, gref = LC.channels(c, d[..., :c['D']], which), LC.channels(c, ref['dlogits'], which)
        grads[which] = H.grad_ratio(g, gref, mode) if np.abs(gref).max() > 0 else float(np.abs(g).max() > 0)
    print('%s: objectives |err| / (1e-04 |ref|) = %s, worst |err| / bound of the channels: %s' % (
        what, ' '.join('%.3f' % r for r in ratios), ' '.join('%s %.3f' % kv for kv in sorted(grads.items()))))
    assert max(ratios) <= 1.0, (what, got, ref['obj'])
    assert all(r <= 1.0 for r in grads.values()), (what, grads)
    g0, r0 = LC.lanes(c, d[..., :c['D']])[..., 0], LC.lanes(c, ref['dlogits'])[..., 0]
    if kw.get('ignore_thresh', 0) > 0:
        ign = ref['aux']['ignored']
        assert np.all(g0[ign] == 0), (what, 'an ignored lane has an objectness gradient')
        live = np.abs(r0) > H.F32_FLOOR * np.abs(r0).max()          # (above the floor of the gradient bound: a zero there is no underflow)
        assert np.all(g0[~ign & live] != 0), (what, 'a lane the specification keeps was ignored')
    # what the options do not concern: the bits of yolo2_loss (of yolo2_loss_box where a box loss is part of the configuration)
    base_objs, base_dl = base(name, mode, kw.get('box_loss', 'mse'))
    for i in range(4):
        if i not in obj_idx or (i == 2 and 'box' in chans):
            assert got[i].tobytes() == base_objs[i].tobytes(), (what, i, got, base_objs)
    bd = base_dl.reshape(c['B'], c['ch'], c['cw'], c['ld'])
    mb = ref['aux']['mask_best'] != 0
    for which in ('obj', 'box', 'cls'):
        if which not in chans or which == 'box':
            assert np.array_equal(bits(LC.channels(c, d[..., :c['D']], which)), bits(LC.channels(c, bd[..., :c['D']], which))), (what, which)
    if 'obj' in chans:       # channel 0 keeps its bits on every lane that is neither ignored nor (with rescore) responsible
        keep = ~ref['aux']['ignored'] & ~(mb & bool(kw.get('rescore')))
        assert np.array_equal(bits(g0[keep]), bits(LC.lanes(c, bd[..., :c['D']])[..., 0][keep])), what


@pytest.mark.parametrize('name,mode', THREE)
def test_default_options_through_the_new_entries_are_the_old_entries(ops, base, name, mode):
    for box_loss in ('mse', 'iou', 'giou', 'diou', 'ciou'):
        base_objs, base_dl = base(name, mode, box_loss)
        objs, dl, _, _ = run(ops, name, mode, dict(box_loss=box_loss))
        assert host(objs).tobytes() == base_objs.tobytes() and np.array_equal(bits(host(dl)), bits(base_dl)), box_loss
        old_objs, old_dl, _, _ = run(ops, name, mode, dict(box_loss=box_loss), split=True, entry='old' if box_loss == 'mse' else 'box')
        objs, dl, _, _ = run(ops, name, mode, dict(box_loss=box_loss), split=True)
        assert same_bits(objs, old_objs) and same_bits(dl, old_dl, mode) and np.array_equal(bits(host(dl)), bits(base_dl)), box_loss


@pytest.mark.parametrize('name,mode', THREE + [('g2x3', 'f32'), ('dense19', 'bf16')])
def test_partials_then_objectives_equals_the_one_call_form_and_repeats(ops, name, mode):
    kw = LC.CONFIGS['all6']
    objs, dl, ws, buf = run(ops, name, mode, kw)
    objs2, dl2, _, _ = run(ops, name, mode, kw, split=True)
    assert same_bits(objs, objs2) and same_bits(dl, dl2, mode)
    objs3, dl3, _, _ = run(ops, name, mode, kw, ws=ws, dl=buf)          # a second launch on the same buffers
    assert same_bits(objs, objs3) and same_bits(dl, dl3, mode)


@pytest.mark.parametrize('mode', H.MODES)
def test_reuses_workspace_and_gradient_buffer_of_a_larger_grid(ops, mode):
    """After the 91-workgroup case both buffers are handed, as they are, to the 13x13 case."""
    kw = LC.CONFIGS['all6']
    _, _, ws, buf = run(ops, 'b8_19x19', 'bf16', kw)
    if mode == 'f32':
        buf = buf.float()
    fresh_objs, fresh_dl, _, _ = run(ops, 'sq13_ld136', mode, kw)
    for split in (False, True):
        objs, dl, _, _ = run(ops, 'sq13_ld136', mode, kw, split=split, ws=ws, dl=buf)
        assert same_bits(objs, fresh_objs) and same_bits(dl, fresh_dl, mode)


BAD = [dict(size=0), dict(size=32), dict(box_loss_code=5), dict(class_loss=3), dict(class_loss=-1), dict(rescore=2), dict(ignore_thresh=1.0),
       dict(ignore_thresh=-0.1), dict(ignore_thresh=float('nan')), dict(ignore_thresh=float('inf')), dict(label_smoothing=1.0, class_loss='ce'),
       dict(label_smoothing=-0.1, class_loss='ce'), dict(label_smoothing=float('nan'), class_loss='ce'), dict(label_smoothing=0.1),
       dict(class_loss='focal', focal_gamma=0.5), dict(class_loss='focal', focal_gamma=-1.0), dict(class_loss='focal', focal_gamma=float('nan')),
       dict(class_loss='focal', focal_gamma=float('inf')), None]


def test_refusals_leave_the_outputs_untouched(ops):
    from yolo_tf_amd._lib import HipKernelError, call, dtype_code, ptr
    c = LC.case('a3')
    B, ch, cw, A, C, ld = c['B'], c['ch'], c['cw'], c['A'], c['C'], c['ld']
    logits = upload(pad_channels(c['net'], ld), 'f32')
    labels = [dev(l.reshape(B, ch * cw, -1)) for l in c['labels']]
    anchors = dev(c['anchors'])
    hp = (ctypes.c_float * 4)(*H.HPARAM)
    for bad in BAD:
        objs, dl, ws = nans(4), nans(B * ch * cw * ld), nans(ops.loss_ws_floats(B, ch * cw, A))
        if bad is None:
            opt = None
        else:
            opt = options(ops, **{k: v for k, v in bad.items() if k != 'box_loss_code'})
            if 'box_loss_code' in bad:
                opt.box_loss = bad['box_loss_code']
        ref = ctypes.byref(opt) if opt is not None else None
        head = [ptr(logits), ld, ptr(anchors)] + [ptr(l) for l in labels] + [hp]
        tail = [ptr(dl), ptr(ws), B, ch, cw, A, C, dtype_code(logits.dtype), ops._stream(), ref]
        with pytest.raises(HipKernelError, match='argument check failed'):
            call('yolo2_loss_ex', *(head + [ptr(objs)] + tail))
        with pytest.raises(HipKernelError, match='argument check failed'):
            call('yolo2_loss_ex_partials', *(head + tail))
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (objs, dl, ws)), bad


@pytest.mark.parametrize('config', ALONE + ['all6'])
def test_ops_wrappers_reach_the_same_kernel(ops, config):
    kw = LC.CONFIGS[config]
    for split in (False, True):
        objs, dl, _, _ = run(ops, 'placed', 'f32', kw, split=split, entry='ops')
        ref_objs, ref_dl, _, _ = run(ops, 'placed', 'f32', kw, split=split)
        assert same_bits(objs, ref_objs) and same_bits(dl, ref_dl)
    c = LC.case('a1')
    t = nans(4)
    for bad, name in ((dict(class_loss='bce'), 'class_loss'), (dict(ignore_thresh=1.5), 'ignore_thresh'), (dict(label_smoothing=0.1), 'label_smoothing'),
                      (dict(class_loss='focal', focal_gamma=0.5), 'focal_gamma'), (dict(rescore=2), 'rescore')):
        with pytest.raises(ValueError, match=name):       # on the host, before any pointer is looked at
            ops.loss(None, 0, None, [None] * 6, H.HPARAM, t, None, None, c['B'], c['ch'], c['cw'], c['A'], c['C'], **bad)
