"""The IoU-family box losses on the device (csrc/head.hip loss_kernel<T, MODE>, csrc/box_loss.h; entries yolo2_loss_box and
yolo2_loss_box_partials) in f32 and bf16 against the float64 specification tests/box_loss_ref.py, on the cases of tests/box_loss_cases.py.
The cases' own conditions and the proof that these bounds catch wrong losses are in tests/test_box_loss_cpu.py.

Bounds: objectives 1e-4 relative (head_cases.objective_ratio); channels 1..4 of dlogits head_cases.f32_ratio in f32 and bf16_ratio in bf16;
everything the option does not concern -- objectives 0, 1 and 3, channel 0 and the class channels of dlogits -- bit-equal to what yolo2_loss
writes for the same inputs.  Every output buffer and the workspace start out filled with NaN."""
import numpy as np
import pytest
import torch

import box_loss_cases as BC
import head_cases as H
from oracle import yolo2_ref as R
from test_head_gpu import TDTYPE, nans, upload
from test_kernels_gpu import dev, host, pad_channels

pytestmark = pytest.mark.gpu

BITS = {'f32': torch.int32, 'bf16': torch.int16}
THREE = [('sq13_ld136', 'f32'), ('sq13_ld136', 'bf16'), ('rect9x14', 'f32'), ('rect9x14', 'bf16'), ('b8_19x19', 'bf16')]


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def run(ops, name, mode, box_loss, split=False, ws=None, dl=None, entry='box', net=None):
    """One launch on NaN-filled outputs (or on the buffers handed in, as they are).  entry 'old': yolo2_loss / yolo2_loss_partials (ops with
    box_loss 'mse'); 'box': yolo2_loss_box / yolo2_loss_box_partials called directly, whatever the mode.  ``net``: other logits for the case's labels.  Returns (objectives, dlogits, ws, dl buffer)."""
    c = BC.case(name)
    B, ch, cw, A, C, ld = c['B'], c['ch'], c['cw'], c['A'], c['C'], c['ld']
    cells = ch * cw
    logits = upload(pad_channels(c['net'] if net is None else net, ld), mode)
    labels = [dev(l.reshape(B, cells, -1)) for l in c['labels']]
    anchors = dev(c['anchors'])
    n = B * cells * ld
    ws = nans(ops.loss_ws_floats(B, cells, A)) if ws is None else ws
    dl = nans(n, TDTYPE[mode]) if dl is None else dl
    objs = nans(4)
    if entry == 'old':
        assert box_loss == 'mse'
        if split:
            ops.loss_partials(logits, ld, anchors, labels, H.HPARAM, dl, ws, B, ch, cw, A, C)
        else:
            ops.loss(logits, ld, anchors, labels, H.HPARAM, objs, dl, ws, B, ch, cw, A, C)
    else:
        import ctypes
        from yolo_tf_amd._lib import BOX_LOSSES, call, dtype_code, ptr
        hp = (ctypes.c_float * 4)(*H.HPARAM)
        args = [ptr(logits), ld, ptr(anchors)] + [ptr(l) for l in labels] + [hp]
        tail = [ptr(dl), ptr(ws), B, ch, cw, A, C, dtype_code(logits.dtype), ops._stream(), BOX_LOSSES[box_loss]]
        if split:
            call('yolo2_loss_box_partials', *(args + tail))
        else:
            call('yolo2_loss_box', *(args + [ptr(objs)] + tail))
    if split:
        ops.loss_objectives(ws, objs, B, ch, cw, A)
    torch.cuda.synchronize()
    return objs, dl[:n].clone(), ws, dl


@pytest.fixture(scope='module')
def mse(ops):
    """What yolo2_loss writes for a case and dtype, once per module."""
    cache = {}

    def get(name, mode):
        if (name, mode) not in cache:
            objs, dl, _, _ = run(ops, name, mode, 'mse', entry='old')
            cache[(name, mode)] = (host(objs), dl)
        return cache[(name, mode)]
    return get


def same_bits(a, b, mode='f32'):
    return torch.equal(a.view(BITS[mode]), b.view(BITS[mode]))


@pytest.mark.parametrize('name,mode,method', BC.ALL)
def test_kernel_vs_specification(ops, mse, name, mode, method):
    c, ref = BC.case(name), BC.reference(name, mode, method)
    objs, dl, _, _ = run(ops, name, mode, method)
    got, d = host(objs), host(dl).reshape(c['B'], c['ch'], c['cw'], c['ld'])
    what = 'box loss %s %s %s' % (name, mode, method)
    ratios = [H.objective_ratio(got[i], ref['obj'][k]) for i, k in enumerate(R.OBJECTIVE_KEYS)]
    g, gref = BC.box_channels(c, d[..., :c['D']]), BC.box_channels(c, ref['dlogits'])
    r_grad = H.grad_ratio(g, gref, mode) if np.abs(gref).max() > 0 else float(np.abs(g).max() > 0)
    print('%s: objectives |err| / (1e-04 |ref|) = %s, channels 1..4 worst |err| / bound = %.3f' % (what, ' '.join('%.3f' % r for r in ratios), r_grad))
    assert np.all(np.isfinite(got)) and not np.isnan(d).any(), what
    assert max(ratios) <= 1.0, (what, got, ref['obj'])
    assert r_grad <= 1.0, (what, r_grad)
    assert np.all(d[..., c['D']:] == 0), 'padding channels of dlogits'
    # what the option does not concern: the bits of yolo2_loss
    base_objs, base_dl = mse(name, mode)
    assert all(got[i].tobytes() == base_objs[i].tobytes() for i in (0, 1, 3)), (what, got, base_objs)
    base = host(base_dl).reshape(c['B'], c['ch'], c['cw'], c['ld'])[..., :c['D']]
    assert np.array_equal(BC.other_channels(c, d[..., :c['D']]).view(np.uint32), BC.other_channels(c, base).view(np.uint32)), what
    if name == 'disjoint' and method == 'iou':
        assert np.all(g == 0)            # IoU exactly 0 for every anchor: nothing pulls


@pytest.mark.parametrize('name,mode', THREE)
def test_mse_through_the_new_entries_is_the_old_loss(ops, mse, name, mode):
    base_objs, base_dl = mse(name, mode)
    objs, dl, _, _ = run(ops, name, mode, 'mse', entry='box')
    assert host(objs).tobytes() == base_objs.tobytes() and same_bits(dl, base_dl, mode)
    old_objs, old_dl, _, _ = run(ops, name, mode, 'mse', split=True, entry='old')
    objs, dl, _, _ = run(ops, name, mode, 'mse', split=True, entry='box')
    assert same_bits(objs, old_objs) and same_bits(dl, old_dl, mode) and same_bits(dl, base_dl, mode)


@pytest.mark.parametrize('name,mode', THREE)
def test_ciou_partials_then_objectives_equals_the_one_call_form_and_repeats(ops, name, mode):
    objs, dl, ws, buf = run(ops, name, mode, 'ciou')
    objs2, dl2, _, _ = run(ops, name, mode, 'ciou', split=True)
    assert same_bits(objs, objs2) and same_bits(dl, dl2, mode)
    objs3, dl3, _, _ = run(ops, name, mode, 'ciou', ws=ws, dl=buf)          # a second launch on the same buffers
    assert same_bits(objs, objs3) and same_bits(dl, dl3, mode)


@pytest.mark.parametrize('mode', H.MODES)
def test_ciou_reuses_workspace_and_gradient_buffer_of_a_larger_grid(ops, mode):
    """As tests/test_head_gpu.py does for mse: after the 91-workgroup case both buffers are handed, as they are, to the 13x13 case."""
    _, _, ws, buf = run(ops, 'b8_19x19', 'bf16', 'ciou')
    if mode == 'f32':
        buf = buf.float()
    fresh_objs, fresh_dl, _, _ = run(ops, 'sq13_ld136', mode, 'ciou')
    for split in (False, True):
        objs, dl, _, _ = run(ops, 'sq13_ld136', mode, 'ciou', split=split, ws=ws, dl=buf)
        assert same_bits(objs, fresh_objs) and same_bits(dl, fresh_dl, mode)


@pytest.mark.parametrize('mode', H.MODES)
def test_a_box_that_underflowed_to_nothing_leaves_the_gradient_finite(ops, mode):
    """Size logits of -800 in every object cell of `a1` (one anchor: responsible): expf gives 0 x 0 boxes.  Every mode's outputs are finite,
    the size channels exactly zero, and objectives and centre gradients are the specification's."""
    import box_loss_ref as S
    c = BC.case('a1')
    net = BC.zero_box_net(c, -800.0).astype(np.float32)       # (exp underflows in float64 too, so the reference sees the same 0 x 0 boxes)
    for method in BC.METHODS:
        obj, aux, ref = S.loss(H.inputs64(net, mode), c['labels'], c['anchors'], H.HP, c['C'], method)
        objs, dl, _, _ = run(ops, 'a1', mode, method, net=net)
        got, d = host(objs), host(dl).reshape(c['B'], c['ch'], c['cw'], c['ld'])
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(d)), method
        g, gref = BC.box_channels(c, d[..., :c['D']]), BC.box_channels(c, ref)
        assert np.all(g[..., 2:] == 0) and np.all(gref[..., 2:] == 0)
        assert H.objective_ratio(got[2], obj['coords']) <= 1.0 and (np.abs(gref).max() == 0 or H.grad_ratio(g, gref, mode) <= 1.0), method


def test_ops_wrappers_and_unknown_modes(ops):
    """ops.loss(box_loss=...) reaches the same kernel as the direct call; an unknown mode is refused on the host."""
    c = BC.case('inside')
    B, ch, cw, A, C, ld = c['B'], c['ch'], c['cw'], c['A'], c['C'], c['ld']
    logits = upload(pad_channels(c['net'], ld), 'f32')
    labels = [dev(l.reshape(B, ch * cw, -1)) for l in c['labels']]
    anchors = dev(c['anchors'])
    objs, dl, ws = nans(4), nans(B * ch * cw * ld), nans(ops.loss_ws_floats(B, ch * cw, A))
    ops.loss(logits, ld, anchors, labels, H.HPARAM, objs, dl, ws, B, ch, cw, A, C, box_loss='giou')
    torch.cuda.synchronize()
    ref_objs, ref_dl, _, _ = run(ops, 'inside', 'f32', 'giou')
    assert same_bits(objs, ref_objs) and same_bits(dl, ref_dl)
    with pytest.raises(ValueError, match='box_loss'):
        ops.loss(logits, ld, anchors, labels, H.HPARAM, objs, dl, ws, B, ch, cw, A, C, box_loss='l1')
    import ctypes
    from yolo_tf_amd._lib import HipKernelError, call, ptr
    hp = (ctypes.c_float * 4)(*H.HPARAM)
    for bad in (-1, 5):
        with pytest.raises(HipKernelError, match='argument check failed'):
            call('yolo2_loss_box', ptr(logits), ld, ptr(anchors), *[ptr(l) for l in labels], hp, ptr(objs), ptr(dl), ptr(ws), B, ch, cw, A, C, 0, ops._stream(), bad)
