"""The head kernels (csrc/head.hip: loss_kernel, loss_finalize_kernel, decode_kernel, decode_attrs_kernel; csrc/yolo1.hip: yolo1_loss_kernel,
yolo1_decode_kernel) in f32 AND bf16 against the float64 oracle on exactly the values they read, on the cases of tests/head_cases.py:
non-square grids, 1 to 33 anchors (lane groups of 1 to 64), padding tails, big logits, exact IoU ties, 91 workgroups.  The inputs'
own conditions (no near-tie anywhere, the number of responsible anchors per cell) and the proof that these bounds catch a subtly
wrong kernel are in tests/test_head_cases_cpu.py.

Bounds: objectives 1e-4 relative in both dtypes (f32 arithmetic on the rounded logits); dlogits in f32 assert_close(F32_RTOL); dlogits
in bf16 per element (2^-8 + 1e-4) |ref| + 1e-5 max|ref| (head_cases.bf16_ratio: half an ulp of a round-to-nearest store, derived);
decode outputs assert_close(F32_RTOL).  Every output buffer and the workspace start out filled with NaN."""
import numpy as np
import pytest
import torch

import head_cases as H
from oracle import yolo2_ref as R
from test_kernels_gpu import assert_close, dev, host, pad_channels, bf16_round, F32_RTOL   # noqa: E402

pytestmark = pytest.mark.gpu

assert F32_RTOL == H.F32_RTOL
TDTYPE = {'f32': torch.float32, 'bf16': torch.bfloat16}
V2 = [(n, m) for n in H.V2_SPECS for m in H.V2_SPECS[n][8]]
V2_DECODE = [(n, m) for n in H.V2_DECODE_CASES for m in H.MODES]
V1 = [(n, m) for n in H.V1_SPECS for m in H.MODES]


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def nans(n, dtype=torch.float32):
    return torch.full((int(n),), float('nan'), dtype=dtype, device='cuda')


def upload(x, mode):
    """Logits on the device in the kernel's dtype; in bf16 mode rounded on the host first, by the rounding the reference used."""
    if mode == 'bf16':
        x = bf16_round(x)
        assert np.array_equal(x, R.bf16_round(x), equal_nan=True)
    return dev(x, TDTYPE[mode])


def check_objectives(got, ref, what):
    ratios = [H.objective_ratio(got[i], ref[k]) for i, k in enumerate(R.OBJECTIVE_KEYS)]
    print('%s: objectives worst |err| / (1e-04 |ref|) = %.3f' % (what, max(ratios)))
    assert np.all(np.isfinite(got)) and max(ratios) <= 1.0, (what, got, ref)


def check_gradient(got, ref, mode, what):
    assert not np.isnan(got).any(), what
    if mode == 'f32':
        assert_close(got, ref, F32_RTOL, what + ' dlogits')
    else:
        ratio = H.bf16_ratio(got, ref)
        print('%s dlogits: worst |err| / ((2^-8 + 1e-04) |ref| + 1e-05 scale) = %.3f' % (what, ratio))
        assert ratio <= 1.0, (what, ratio)


# ---------------------------------------------------------------------------------------------------------------------
# YOLOv2 loss
# ---------------------------------------------------------------------------------------------------------------------

def v2_device_inputs(name, mode):
    c = H.v2_case(name)
    cells = c['ch'] * c['cw']
    logits = upload(pad_channels(c['net'], c['ld']), mode)
    labels = [dev(l.reshape(c['B'], cells, -1)) for l in c['labels']]
    return c, logits, labels, dev(c['anchors'])


def run_v2_loss(ops, name, mode, split=False, ws=None, dl=None):
    """One launch of the loss on NaN-filled outputs (or on the buffers handed in, as they are).  Returns (objectives, dlogits, ws, dl buffer)."""
    c, logits, labels, anchors = v2_device_inputs(name, mode)
    B, ch, cw, A, C, ld = c['B'], c['ch'], c['cw'], c['A'], c['C'], c['ld']
    n = B * ch * cw * ld
    ws = nans(ops.loss_ws_floats(B, ch * cw, A)) if ws is None else ws
    dl = nans(n, TDTYPE[mode]) if dl is None else dl
    objs = nans(4)
    if split:
        ops.loss_partials(logits, ld, anchors, labels, H.HPARAM, dl, ws, B, ch, cw, A, C)
        ops.loss_objectives(ws, objs, B, ch, cw, A)
    else:
        ops.loss(logits, ld, anchors, labels, H.HPARAM, objs, dl, ws, B, ch, cw, A, C)
    torch.cuda.synchronize()
    return objs, dl[:n].clone(), ws, dl


@pytest.mark.parametrize('name,mode', V2)
def test_v2_loss_vs_oracle(ops, name, mode):
    c, ref = H.v2_case(name), H.v2_reference(name, mode)
    objs, dl, _, _ = run_v2_loss(ops, name, mode)
    what = 'v2 loss %s %s' % (name, mode)
    check_objectives(host(objs), ref['obj'], what)
    d = host(dl).reshape(c['B'], c['ch'], c['cw'], c['ld'])
    assert np.all(d[..., c['D']:] == 0), 'padding channels of dlogits'
    check_gradient(d[..., :c['D']], ref['dlogits'], mode, what)


@pytest.mark.parametrize('name,mode', [('sq13_ld136', 'f32'), ('sq13_ld136', 'bf16'), ('rect9x14', 'f32'), ('rect9x14', 'bf16'), ('b8_19x19', 'bf16')])
def test_v2_loss_partials_then_objectives_equals_loss(ops, name, mode):
    """The pair the training session calls (yolo2_loss_partials on the step, yolo2_loss_objectives when a summary is due), bit for bit."""
    objs, dl, _, _ = run_v2_loss(ops, name, mode)
    objs2, dl2, _, _ = run_v2_loss(ops, name, mode, split=True)
    assert torch.equal(objs.view(torch.int32), objs2.view(torch.int32))
    assert torch.equal(dl.view(torch.int16 if mode == 'bf16' else torch.int32), dl2.view(torch.int16 if mode == 'bf16' else torch.int32))
    check_objectives(host(objs2), H.v2_reference(name, mode)['obj'], 'v2 partials+objectives %s %s' % (name, mode))


@pytest.mark.parametrize('mode', H.MODES)
def test_v2_loss_reuses_workspace_and_gradient_buffer_of_a_larger_grid(ops, mode):
    """The session keeps one workspace and one gradient buffer across steps and grid sizes: after the 91-workgroup case both are handed,
    as they are, to the 13x13 case; nothing of the earlier launch may show."""
    _, _, ws, buf = run_v2_loss(ops, 'b8_19x19', 'bf16')
    if mode == 'f32':
        buf = buf.float()       # (the values of the bf16 run, in the dtype this launch writes)
    fresh_objs, fresh_dl, _, _ = run_v2_loss(ops, 'sq13_ld136', mode)
    for split in (False, True):
        objs, dl, _, _ = run_v2_loss(ops, 'sq13_ld136', mode, split=split, ws=ws, dl=buf)
        assert torch.equal(objs.view(torch.int32), fresh_objs.view(torch.int32))
        assert torch.equal(dl.view(torch.int16 if mode == 'bf16' else torch.int32), fresh_dl.view(torch.int16 if mode == 'bf16' else torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# YOLOv2 decode
# ---------------------------------------------------------------------------------------------------------------------

def run_v2_decode(ops, c, logits, anchors):
    B, ch, cw, A, C, ld = c['B'], c['ch'], c['cw'], c['A'], c['C'], c['ld']
    n = B * ch * cw * A
    conf, mn, mx, flag = nans(n * C), nans(n * 2), nans(n * 2), torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.head_decode(logits, ld, anchors, conf, mn, mx, flag, B, ch, cw, A, C)
    torch.cuda.synchronize()
    return conf, mn, mx, int(flag.item())


@pytest.mark.parametrize('name,mode', V2_DECODE)
def test_v2_decode_vs_oracle(ops, name, mode):
    c, logits, _, anchors = v2_device_inputs(name, mode)
    B, ch, cw, A, C, ld = c['B'], c['ch'], c['cw'], c['A'], c['C'], c['ld']
    m = H.v2_reference(name, mode)['m']
    n = B * ch * cw * A
    conf, mn, mx, flag = run_v2_decode(ops, c, logits, anchors)
    assert flag == 0
    sizes = {'iou': n, 'prob': n * C, 'xy': n * 2, 'wh': n * 2}
    full = {k: nans(v) for k, v in sizes.items()}
    ops.head_decode_attrs(logits, ld, anchors, full['iou'], full['prob'], full['xy'], full['wh'], B, ch, cw, A, C)
    torch.cuda.synchronize()
    what = 'v2 decode %s %s ' % (name, mode)
    for key, t in (('conf', conf), ('xy_min', mn), ('xy_max', mx), ('iou', full['iou']), ('prob', full['prob']), ('xy', full['xy']), ('wh', full['wh'])):
        got = host(t).reshape(m[key].shape)
        assert np.all(np.isfinite(got)), key
        assert_close(got, m[key], F32_RTOL, what + key)
    # any single output alone (the others NULL): the same bits
    for key in sizes:
        one = nans(sizes[key])
        args = {k: (one if k == key else None) for k in sizes}
        ops.head_decode_attrs(logits, ld, anchors, args['iou'], args['prob'], args['xy'], args['wh'], B, ch, cw, A, C)
        torch.cuda.synchronize()
        assert torch.equal(one.view(torch.int32), full[key].view(torch.int32)), key


@pytest.mark.parametrize('mode', H.MODES)
def test_v2_decode_flag(ops, mode):
    """tf.check_numerics counterpart: a NaN class logit raises the flag; an objectness logit of -inf does not (sigmoid(-inf) = 0, conf = 0, as in the reference)."""
    name = 'rect9x14'
    c = H.v2_case(name)
    B, ch, cw, A, C, D = c['B'], c['ch'], c['cw'], c['A'], c['C'], c['D']
    anchors = dev(c['anchors'])
    d = 5 + C
    bad = c['net'].copy()
    bad[1, 4, 9, 2 * d + 5 + 17] = np.nan           # image 1, row 4, column 9, anchor 2, class 17
    conf, mn, mx, flag = run_v2_decode(ops, c, upload(pad_channels(bad, c['ld']), mode), anchors)
    assert flag != 0
    got = host(conf).reshape(B, ch * cw, A, C)
    assert np.isnan(got[1, 4 * cw + 9, 2]).all()
    got[1, 4 * cw + 9, 2] = 0
    assert np.all(np.isfinite(got))                  # that box only
    low = c['net'].copy()
    low[2, 8, 13, 4 * d] = -np.inf                   # the last cell's last anchor
    conf, mn, mx, flag = run_v2_decode(ops, c, upload(pad_channels(low, c['ld']), mode), anchors)
    assert flag == 0
    got = host(conf).reshape(B, ch * cw, A, C)
    assert np.all(got[2, -1, 4] == 0)
    ref = H.v2_reference(name, mode)['m']
    keep = np.ones((B, ch * cw, A), bool)
    keep[2, -1, 4] = False
    assert_close(got[keep], ref['conf'][keep], F32_RTOL, 'v2 decode -inf objectness %s conf elsewhere' % mode)
    assert_close(host(mn).reshape(ref['xy_min'].shape), ref['xy_min'], F32_RTOL, 'v2 decode -inf objectness %s xy_min' % mode)


# ---------------------------------------------------------------------------------------------------------------------
# YOLO (v1)
# ---------------------------------------------------------------------------------------------------------------------

def v1_device_inputs(name, mode):
    c = H.v1_case(name)
    return c, upload(pad_channels(c['net'], c['ld']), mode).reshape(-1), [dev(l) for l in c['labels']]


@pytest.mark.parametrize('name,mode', V1)
def test_v1_loss_vs_oracle(ops, name, mode):
    c, net, labels = v1_device_inputs(name, mode)
    B, ch, cw, boxes, C, ld, width = c['B'], c['ch'], c['cw'], c['boxes'], c['C'], c['ld'], c['width']
    ref = H.v1_reference(name, mode)
    objs, dnet, ws = nans(4), nans(B * ld, TDTYPE[mode]), nans(ops.loss_ws_floats(B, ch * cw, boxes))
    ops.yolo1_loss(net, ld, labels, H.HPARAM, objs, dnet, ws, B, ch, cw, boxes, C)
    torch.cuda.synchronize()
    what = 'v1 loss %s %s' % (name, mode)
    check_objectives(host(objs), ref['obj'], what)
    d = host(dnet).reshape(B, ld)
    assert np.all(d[:, width:] == 0), 'padding of dnet'
    check_gradient(d[:, :width], ref['dnet'], mode, what)
    # the |x| gradient at 0 is 0 for the responsible boxes of that cell, exactly
    b, cell = c['zero_cell']
    at = ch * cw * C + (cell * boxes + np.arange(boxes)) * 5 + 3
    assert np.all(ref['dnet'][b, at] == 0) and np.all(d[b, at] == 0)


@pytest.mark.parametrize('name,mode', V1)
def test_v1_decode_vs_oracle(ops, name, mode):
    c, net, _ = v1_device_inputs(name, mode)
    B, ch, cw, boxes, C, ld = c['B'], c['ch'], c['cw'], c['boxes'], c['C'], c['ld']
    m = H.v1_reference(name, mode)['m']
    n = B * ch * cw * boxes

    def run(logits):
        conf, mn, mx, flag = nans(n * C), nans(n * 2), nans(n * 2), torch.zeros(1, dtype=torch.int32, device='cuda')
        ops.yolo1_head_decode(logits, ld, conf, mn, mx, flag, B, ch, cw, boxes, C)
        torch.cuda.synchronize()
        return conf, mn, mx, int(flag.item())

    conf, mn, mx, flag = run(net)
    assert flag == 0
    what = 'v1 decode %s %s ' % (name, mode)
    for key, t in (('conf', conf), ('xy_min', mn), ('xy_max', mx)):
        ref = np.broadcast_to(m[key], (B, ch * cw, boxes, m[key].shape[-1]))
        got = host(t).reshape(ref.shape)
        assert np.all(np.isfinite(got)), key
        assert_close(got, ref, F32_RTOL, what + key)
    bad = pad_channels(c['net'], ld).copy()
    bad[B - 1, (ch * cw - 1) * C + 1] = np.nan           # the last cell's class 1 in the last image
    conf, _, _, flag = run(upload(bad, mode).reshape(-1))
    assert flag != 0
    got = host(conf).reshape(B, ch * cw, boxes, C)
    assert np.isnan(got[B - 1, -1, :, 1]).all() and np.isnan(got).sum() == boxes
