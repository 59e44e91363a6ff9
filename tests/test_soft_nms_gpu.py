"""yolo2_soft_nms (csrc/soft_nms.hip) against its specification (tests/soft_nms_ref.py) on the cases of tests/soft_nms_cases.py, for the linear
and the Gaussian decay: scores as uint32 bit patterns (zeros keep their sign, untouched scores their bits), boxes untouched, the order element
by element.  conf and order are slices of larger buffers with 64 sentinel elements on either side.  What each case exercises, and the proof
that a subtly wrong kernel fails some of them, is in tests/test_soft_nms_cpu.py.

Method hard through this kernel is compared with yolo2_nms (ops.nms) on the tie-free cases: every candidate's score bit for bit; a score that
is not above the threshold is untouched here, while yolo2_nms, as the reference does, writes +0 into it if the box overlaps a kept one (see
tests/test_soft_nms_cpu.py) -- where it did not, all bits are equal.

The order of ORDER matters: small sizes, then N = 4096, then small sizes again, then N = 2728 / 2727 / 4095, so that the per-device bookkeeping
of the raised LDS limit sees growing, shrinking and re-growing requests."""
import numpy as np
import pytest
import torch

import soft_nms_cases as M

pytestmark = pytest.mark.gpu

GUARD = 64
CONF_GUARD, ORDER_GUARD = 0x7FC0BEEF, -0x0BADBEEF
_SIZE_NAMES = ['n%d' % n for n in M.SIZES]
_BIG = ['n4096', 'chain4096']
ORDER = ([n for n in _SIZE_NAMES if M.CASES[n][1] <= 1025] + _BIG + [n for n in M.NAMES if n not in _SIZE_NAMES + _BIG] + ['n2728', 'n2727', 'n4095'])
assert sorted(ORDER) == sorted(M.NAMES)
TIE_FREE = [n for n in ORDER if n != 'nan_scores' and M.tie_free(n)]


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    return _ops


def guarded(n, dtype, fill):
    """(whole buffer, the n elements between the guards)."""
    whole = torch.full((GUARD + n + GUARD,), fill, dtype=torch.int32, device='cuda')
    return whole, whole[GUARD:GUARD + n].view(dtype)


def guards_intact(whole, n, fill):
    return bool((whole[:GUARD] == fill).all().item()) and bool((whole[GUARD + n:] == fill).all().item())


def launch(ops, conf, mn, mx, method, thr, thr_iou, sigma, with_order, stream=None):
    """One call of ops.soft_nms on fresh guarded buffers.  conf [B,N,C], mn / mx [B,N,2] (NumPy f32).  Returns (conf bits [B,N,C] uint32,
    order [B,N] or None), after asserting that the boxes, every guard and (without an order) the order buffer are untouched."""
    B, N, C = conf.shape
    conf_whole, conf_d = guarded(B * N * C, torch.float32, CONF_GUARD)
    order_whole, order_d = guarded(B * N, torch.int32, ORDER_GUARD)
    conf_d.view(torch.int32).copy_(torch.from_numpy(M.bits(conf).view(np.int32).reshape(-1).copy()))      # (as integers: NaN payloads stay)
    mn_d, mx_d = torch.from_numpy(mn.copy()).cuda(), torch.from_numpy(mx.copy()).cuda()
    torch.cuda.synchronize()
    if stream is None:
        ops.soft_nms(conf_d, mn_d, mx_d, order_d if with_order else None, B, N, C, method, thr, thr_iou, sigma)
    else:
        with torch.cuda.stream(stream):
            ops.soft_nms(conf_d, mn_d, mx_d, order_d if with_order else None, B, N, C, method, thr, thr_iou, sigma)
    torch.cuda.synchronize()
    assert guards_intact(conf_whole, B * N * C, CONF_GUARD), 'conf guards'
    assert guards_intact(order_whole, B * N, ORDER_GUARD), 'order guards'
    if not with_order:
        assert bool((order_whole == ORDER_GUARD).all().item()), 'a buffer that was not passed'
    assert np.array_equal(M.bits(mn_d.cpu().numpy()), M.bits(mn)) and np.array_equal(M.bits(mx_d.cpu().numpy()), M.bits(mx)), 'boxes'
    got = conf_d.view(torch.int32).cpu().numpy().view(np.uint32).reshape(B, N, C)
    return got, (order_d.cpu().numpy().reshape(B, N) if with_order else None)


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
@pytest.mark.parametrize('name', ORDER)
def test_soft_nms_case_vs_specification(ops, name, method):
    c = M.case(name)
    ref_conf, ref_order = M.reference(name, method)
    stream = torch.cuda.Stream() if name == M.SIDE_STREAM_CASE else None
    args = (method, c['thr'], c['thr_iou'], c['sigma'], c['with_order'])
    got, order = launch(ops, c['conf'], c['xy_min'], c['xy_max'], *args, stream=stream)
    ref_bits = M.bits(ref_conf)
    for b in range(c['B']):
        wrong = np.argwhere(got[b] != ref_bits[b])
        assert len(wrong) == 0, '%s %s image %d: %d scores differ, first (box, class) %s: got %s, want %s' % (
            name, method, b, len(wrong), wrong[:4].tolist(), [hex(got[b][tuple(w)]) for w in wrong[:4]], [hex(ref_bits[b][tuple(w)]) for w in wrong[:4]])
        if c['with_order']:
            assert np.array_equal(order[b], ref_order[b]), '%s image %d: order differs at %s' % (name, b, np.flatnonzero(order[b] != ref_order[b])[:4])
    # the same call on fresh copies: the same bits (an LDS race would show as a difference)
    again, order2 = launch(ops, c['conf'], c['xy_min'], c['xy_max'], *args, stream=stream)
    assert np.array_equal(again, got) and (order is None or np.array_equal(order2, order))
    # the last image alone equals its part of the batch
    if c['B'] > 1:
        b = c['B'] - 1
        one, order1 = launch(ops, c['conf'][b:b + 1], c['xy_min'][b:b + 1], c['xy_max'][b:b + 1], *args, stream=stream)
        assert np.array_equal(one[0], got[b]) and (order is None or np.array_equal(order1[0], order[b])), '%s image %d alone' % (name, b)


def compare_hard(ops, name):
    """Asserts the comparison of the module docstring; returns whether yolo2_nms touched a non-candidate."""
    c = M.case(name)
    B, N, C = c['conf'].shape
    got, _ = launch(ops, c['conf'], c['xy_min'], c['xy_max'], 'hard', c['thr'], c['thr_iou'], c['sigma'], False)
    conf_d = torch.from_numpy(c['conf'].copy()).cuda()
    ws = torch.zeros(ops.workspace_bytes('nms', B, N, C) // 4, dtype=torch.int32, device='cuda')
    ops.nms(conf_d, torch.from_numpy(c['xy_min'].copy()).cuda(), torch.from_numpy(c['xy_max'].copy()).cuda(), None, ws, B, N, C, c['thr'], c['thr_iou'])
    torch.cuda.synchronize()
    hard = M.bits(conf_d.cpu().numpy())
    before = M.bits(c['conf'])
    cand = c['conf'] > np.float32(c['thr'])
    assert np.array_equal(got[cand], hard[cand]), '%s: %d candidates differ' % (name, int((got[cand] != hard[cand]).sum()))
    assert np.array_equal(got[~cand], before[~cand]), 'a non-candidate was touched'
    touched = hard[~cand] != before[~cand]
    assert np.all(hard[~cand][touched] == 0)
    if not touched.any():
        assert np.array_equal(got, hard)
    return bool(touched.any())


@pytest.mark.parametrize('name', TIE_FREE)
def test_hard_through_this_kernel_equals_yolo2_nms_on_tie_free_cases(ops, name):
    compare_hard(ops, name)


def test_hard_equals_yolo2_nms_in_every_bit_where_no_non_candidate_overlaps(ops):
    for name in ('all_candidates', 'all_candidates_n257', 'disjoint'):
        assert name in TIE_FREE and not compare_hard(ops, name), name


def test_device_postprocess_wrappers(ops):
    """utils.postprocess.soft_non_max_suppress_device and the NumPy drop-in beside the existing pair."""
    from yolo_tf_amd.utils import postprocess
    c = M.case('n65')
    for method in ('linear', 'gaussian'):
        ref_conf, ref_order = M.reference('n65', method)
        conf_d = torch.from_numpy(c['conf'].copy()).cuda()
        order = postprocess.soft_non_max_suppress_device(conf_d, torch.from_numpy(c['xy_min'].copy()).cuda(), torch.from_numpy(c['xy_max'].copy()).cuda(),
                                                         c['thr'], c['thr_iou'], method=method, sigma=c['sigma'])
        assert np.array_equal(M.bits(conf_d.cpu().numpy()), M.bits(ref_conf)) and np.array_equal(order.cpu().numpy(), ref_order)
        conf = c['conf'][0].reshape(13, 5, 3).copy()
        boxes = postprocess.soft_non_max_suppress(conf, c['xy_min'][0].reshape(13, 5, 2), c['xy_max'][0].reshape(13, 5, 2), c['thr'], c['thr_iou'], method, c['sigma'])
        assert np.array_equal(M.bits(conf.reshape(65, 3)), M.bits(ref_conf[0]))                   # mutated in place
        assert len(boxes) == 65 and all(np.array_equal(row, ref_conf[0][i]) for (row, _, _), i in zip(boxes, ref_order[0]))
        assert boxes[0][0].base is not None and np.shares_memory(boxes[0][0], conf)                # views into the caller's array


@pytest.mark.parametrize('bad', [dict(N=4097), dict(N=0), dict(B=0), dict(C=0), dict(method=3), dict(thr=-1.0), dict(thr_iou=float('inf')), dict(sigma=0.01)],
                         ids=lambda d: '%s=%s' % next(iter(d.items())))
def test_soft_nms_refuses_what_it_cannot_serve_and_writes_nothing(ops, bad):
    from yolo_tf_amd._lib import HipKernelError
    n = 4097 * 4
    a = dict(dict(B=1, N=64, C=3, method=2, thr=0.3, thr_iou=0.45, sigma=0.5), **bad)
    conf_whole, conf_d = guarded(n, torch.float32, CONF_GUARD)
    order_whole, order_d = guarded(n, torch.int32, ORDER_GUARD)
    rng = np.random.RandomState(7)
    boxes = rng.uniform(0, 5, (n, 2)).astype(np.float32)
    mn_d, mx_d = torch.from_numpy(boxes).cuda(), torch.from_numpy(boxes + np.float32(1)).cuda()
    scores = rng.uniform(0.5, 1, n).astype(np.float32)
    conf_d.copy_(torch.from_numpy(scores))
    torch.cuda.synchronize()
    with pytest.raises(HipKernelError):
        ops.soft_nms(conf_d, mn_d, mx_d, order_d, a['B'], a['N'], a['C'], a['method'], a['thr'], a['thr_iou'], a['sigma'])
    torch.cuda.synchronize()
    assert np.array_equal(M.bits(conf_d.cpu().numpy()), M.bits(scores))
    assert guards_intact(conf_whole, n, CONF_GUARD) and bool((order_whole == ORDER_GUARD).all().item())
