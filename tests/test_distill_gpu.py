"""The distill kernel (csrc/distill.hip: yolo2_distill_partials, yolo2_distill_objectives) against its specification tests/distill_ref.py on the cases
of tests/distill_cases.py, within the project's derived bounds (tests/head_cases.py); accumulation into dlogits, exact zeros, padding, bitwise
reproducibility and argument errors.  Every output and the workspace start out filled with NaN."""
import ctypes

import numpy as np
import pytest
import torch

import distill_cases as D
import distill_ref as S
import head_cases as H
from oracle import yolo2_ref as R
from test_kernels_gpu import dev, host, bf16_round

pytestmark = pytest.mark.gpu

TDTYPE = {'f32': torch.float32, 'bf16': torch.bfloat16}
BITS = {'f32': torch.int32, 'bf16': torch.int16}
ALL = [(n, p, o) for n in D.SPECS for p in D.PAIRS for o in D.OPTIONS]
SOME = [(n, p, o) for n, o in (('pad3x4', 'mse'), ('sq13', 'kl_T2.5'), ('rect9x14', 'mse_T2.5_raw'), ('saturated', 'kl_raw')) for p in D.PAIRS]


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def nans(n, dtype=torch.float32):
    return torch.full((int(n),), float('nan'), dtype=dtype, device='cuda')


def upload(x, ld, mode, pad=float('nan')):
    """[B, cells, A, d] -> device rows of ld channels in the kernel's dtype (bf16 mode: rounded on the host by the reference's rounding); padding channels NaN."""
    B, cells = x.shape[:2]
    rows = np.full((B, cells, ld), pad, np.float32)
    rows[..., :x.shape[2] * x.shape[3]] = x.reshape(B, cells, -1)
    if mode == 'bf16':
        rows = bf16_round(rows)
        assert np.array_equal(rows, R.bf16_round(rows), equal_nan=True)
    return dev(rows, TDTYPE[mode])


def run(ops, name, pair, options, start=None, dl=True, split=True):
    """One launch on NaN-filled objectives and workspace.  ``start``: the real channels dlogits holds before the launch (None: zeros); its padding
    channels hold NaN.  Returns (objectives f32[3] tensor, dlogits tensor [B, cells, ld_s] or None, workspace)."""
    c = D.case(name)
    B, ch, cw, A, C = c['B'], c['ch'], c['cw'], c['A'], c['C']
    s, t = upload(c['s'], c['ld_s'], pair[0]), upload(c['t'], c['ld_t'], pair[1])
    d = upload(np.zeros_like(c['s']) if start is None else start, c['ld_s'], pair[0]) if dl else None
    ws, objs = nans(ops.distill_ws_floats(B, ch * cw, A)), nans(3)
    ops.distill_partials(s, c['ld_s'], t, c['ld_t'], d, ws, B, ch, cw, A, C, **D.OPTIONS[options])
    if split:
        ops.distill_objectives(ws, objs, B, ch, cw, A)
    torch.cuda.synchronize()
    return objs, d, ws


def real(c, d):
    return host(d)[..., :c['D']].reshape(c['s'].shape).astype(np.float64)


@pytest.mark.parametrize('name,pair,options', ALL)
def test_against_the_specification(ops, name, pair, options):
    c = D.case(name)
    ref_obj, ref_g = D.reference(name, pair, options)
    objs, d, ws = run(ops, name, pair, options)
    got = host(objs)
    what = 'distill %s %s/%s %s' % (name, pair[0], pair[1], options)
    ratios = [H.objective_ratio(got[i], ref_obj[k]) for i, k in enumerate(D.KEYS)]
    g = real(c, d)
    ratio = H.grad_ratio(g, ref_g, pair[0])
    print('%s: objectives %s, worst |err| / (1e-04 |ref|) = %.3f; gradient worst |err| / bound = %.3f' % (what, got, max(ratios), ratio))
    assert np.isfinite(got).all() and not np.isnan(host(ws)).any() and np.isfinite(g).all(), what
    assert max(ratios) <= 1.0, (what, got, ref_obj)
    if c['C'] == 1:
        assert got[2] == 0.0 and not g[..., 5:].any(), 'one class: the class term and its gradient are exactly 0'
    assert ratio <= 1.0, (what, ratio)
    pad = d[..., c['D']:]
    assert bool(torch.isnan(pad).all()), 'padding channels of dlogits are untouched'


@pytest.mark.parametrize('name,pair,options', SOME)
def test_accumulates_into_dlogits(ops, name, pair, options):
    c, mode = D.case(name), pair[0]
    _, ref_g = D.reference(name, pair, options)
    d0 = D.start_gradient(name, mode)
    _, zero_start, _ = run(ops, name, pair, options)
    _, d, _ = run(ops, name, pair, options, start=d0)
    out = real(c, d)
    if mode == 'f32':          # one f32 addition separates the two launches
        want = d0 + host(zero_start)[..., :c['D']].reshape(d0.shape)
        assert want.dtype == np.float32
        assert np.array_equal(host(d)[..., :c['D']].reshape(d0.shape).view(np.uint32), want.view(np.uint32))
    ratio = S.accumulate_ratio(out, d0, ref_g, mode)
    print('distill accumulate %s %s/%s %s: worst |out - (d0 + g)| / bound = %.3f' % (name, pair[0], pair[1], options, ratio))
    assert ratio <= 1.0
    assert bool(torch.isnan(d[..., c['D']:]).all()), 'padding channels of dlogits are untouched'


@pytest.mark.parametrize('mode', H.MODES)
@pytest.mark.parametrize('options', ['mse', 'kl_T2.5'])
def test_identical_heads_give_exact_zeros_and_keep_dlogits(ops, mode, options):
    c = D.case('sq13')
    B, ch, cw, A, C = c['B'], c['ch'], c['cw'], c['A'], c['C']
    s = upload(c['s'], c['ld_s'], mode)
    d0 = upload(D.start_gradient('sq13', mode), c['ld_s'], mode)
    d = d0.clone()
    ws, objs = nans(ops.distill_ws_floats(B, ch * cw, A)), nans(3)
    ops.distill_partials(s, c['ld_s'], s.clone(), c['ld_s'], d, ws, B, ch, cw, A, C, **D.OPTIONS[options])
    ops.distill_objectives(ws, objs, B, ch, cw, A)
    torch.cuda.synchronize()
    assert host(objs).tolist() == [0.0, 0.0, 0.0]
    assert torch.equal(d.view(BITS[mode]), d0.view(BITS[mode]))


@pytest.mark.parametrize('name,pair,options', SOME)
def test_reproducible_and_null_dlogits(ops, name, pair, options):
    d0 = D.start_gradient(name, pair[0])
    o1, d1, w1 = run(ops, name, pair, options, start=d0)
    o2, d2, w2 = run(ops, name, pair, options, start=d0)
    bits = BITS[pair[0]]
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(w1.view(torch.int32), w2.view(torch.int32))
    assert torch.equal(d1.view(bits), d2.view(bits))
    o3, none, w3 = run(ops, name, pair, options, dl=False)            # objectives only
    assert none is None and torch.equal(o1.view(torch.int32), o3.view(torch.int32)) and torch.equal(w1.view(torch.int32), w3.view(torch.int32))
    # the partials alone leave the objectives' NaN fill; reducing them again gives the same bits
    c = D.case(name)
    o4, _, w4 = run(ops, name, pair, options, dl=False, split=False)
    assert bool(torch.isnan(o4).all())
    ops.distill_objectives(w4, o4, c['B'], c['ch'], c['cw'], c['A'])
    ops.distill_objectives(w4, o2, c['B'], c['ch'], c['cw'], c['A'])
    torch.cuda.synchronize()
    assert torch.equal(o1.view(torch.int32), o4.view(torch.int32)) and torch.equal(o1.view(torch.int32), o2.view(torch.int32))


def test_argument_errors_launch_nothing(ops):
    from yolo_tf_amd import _lib
    c = D.case('pad3x4')
    B, ch, cw, A, C = c['B'], c['ch'], c['cw'], c['A'], c['C']
    s, t = upload(c['s'], c['ld_s'], 'f32'), upload(c['t'], c['ld_t'], 'f32')
    d, ws, objs = nans(B * ch * cw * c['ld_s']), nans(ops.distill_ws_floats(B, ch * cw, A)), nans(3)
    good = dict(size=ctypes.sizeof(_lib.DistillOptions), class_term=0, scale_by_objectness=1, weight=1.0, w_objectness=1.0, w_coords=1.0, w_prob=1.0, temperature=1.0)
    ptr, stream = _lib.ptr, ops._stream()

    def status(opt=good, student=s, teacher=t, dl=d, w=ws, dtype_s=0, dtype_t=0, ld_s=c['ld_s'], ld_t=c['ld_t'], null_opt=False):
        o = _lib.DistillOptions(**opt)
        return _lib.load().yolo2_distill_partials(ptr(student), ld_s, dtype_s, ptr(teacher), ld_t, dtype_t, ptr(dl), ptr(w), B, ch, cw, A, C, stream,
                                                  None if null_opt else ctypes.byref(o))
    bad = [dict(student=None), dict(teacher=None), dict(w=None), dict(null_opt=True), dict(dtype_s=2), dict(dtype_t=-1), dict(dtype_t=7),
           dict(ld_s=c['D'] - 1), dict(ld_t=c['D'] - 1)]
    bad += [dict(opt=dict(good, **kw)) for kw in (dict(size=good['size'] + 4), dict(size=0), dict(temperature=0.0), dict(temperature=-1.0),
                                                  dict(temperature=float('inf')), dict(temperature=float('nan')), dict(weight=-1.0), dict(w_objectness=-0.5),
                                                  dict(w_coords=-1e-3), dict(w_prob=float('nan')), dict(class_term=2), dict(class_term=-1), dict(scale_by_objectness=2))]
    for kw in bad:
        assert status(**kw) != 0, kw
        assert b'argument check failed' in _lib.load().yolo2_last_error(), kw
    assert _lib.load().yolo2_distill_objectives(None, ptr(objs), B, ch, cw, A, stream) != 0
    assert _lib.load().yolo2_distill_objectives(ptr(ws), None, B, ch, cw, A, stream) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(d).all()) and bool(torch.isnan(ws).all()) and bool(torch.isnan(objs).all())
    for kw in (dict(class_term='ce'), dict(temperature=0), dict(weight=-1), dict(prob=float('nan')), dict(scale_by_objectness=2)):      # the wrapper refuses on the host
        with pytest.raises(ValueError):
            ops.distill_partials(s, c['ld_s'], t, c['ld_t'], d, ws, B, ch, cw, A, C, **kw)
    assert status() == 0          # ... and the good call goes through
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ws).any())
