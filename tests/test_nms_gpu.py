"""yolo2_nms (csrc/nms.hip) against the oracle on the cases of tests/nms_cases.py: sizes around every boundary of the kernel (64-box words,
boxes per thread, the 64 KiB LDS request, the N = 4096 limit), chosen candidate counts, thresholds (negative, -0.0, 0, eval.py's, 1; IoU 0, 1,
above 1), order_out = NULL, C = 1 and 80, a non-default stream, ties whose carried order passes through a suppressed box, zero-area boxes.
What each case exercises, and the proof that a subtly wrong kernel fails some of them, is in tests/test_nms_cases_cpu.py.

Every comparison is exact: scores as uint32 bit patterns (zeros keep their sign, untouched scores their bits), the order element by element.
conf, order and ws are slices of larger buffers with 64 sentinel elements on either side, ws of exactly workspace_bytes('nms', B, N, C).

The order of ORDER matters: small sizes, then N = 4096, then small sizes again, then N = 2011, so that the per-device bookkeeping of the raised
LDS limit sees growing, shrinking and re-growing requests (other tests of the process may have raised it before: only results are asserted)."""
import numpy as np
import pytest
import torch

import nms_cases as M

pytestmark = pytest.mark.gpu

GUARD = 64
CONF_GUARD, ORDER_GUARD, WS_GUARD = 0x7FC0BEEF, -0x0BADBEEF, 0x5EA7ED5
_SIZE_NAMES = ['n%d' % n for n in M.SIZES]
_BIG = ['n4096', 'thr_neg1_n4096']
ORDER = ([n for n in _SIZE_NAMES if M.CASES[n][1] <= 1025] + _BIG + [n for n in M.NAMES if n not in _SIZE_NAMES + _BIG] + ['n2010', 'n2011', 'n4095'])
assert sorted(ORDER) == sorted(M.NAMES)


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


def launch(ops, conf, mn, mx, thr, thr_iou, with_order, stream=None):
    """One call of ops.nms on fresh guarded buffers.  conf [B,N,C], mn / mx [B,N,2] (NumPy f32).  Returns (conf bits [B,N,C] uint32, order
    [B,N] or None), after asserting that the boxes, every guard and (without an order) a bystander buffer are untouched."""
    B, N, C = conf.shape
    ws_bytes = ops.workspace_bytes('nms', B, N, C)
    assert ws_bytes == 4 * B * N * C
    conf_whole, conf_d = guarded(B * N * C, torch.float32, CONF_GUARD)
    order_whole, order_d = guarded(B * N, torch.int32, ORDER_GUARD)
    ws_whole, ws_d = guarded(ws_bytes // 4, torch.int32, WS_GUARD)
    assert ws_d.numel() * ws_d.element_size() == ws_bytes
    conf_d.copy_(torch.from_numpy(conf.reshape(-1).copy()))
    mn_d, mx_d = torch.from_numpy(mn.copy()).cuda(), torch.from_numpy(mx.copy()).cuda()
    torch.cuda.synchronize()
    if stream is None:
        ops.nms(conf_d, mn_d, mx_d, order_d if with_order else None, ws_d, B, N, C, thr, thr_iou)
    else:
        with torch.cuda.stream(stream):
            ops.nms(conf_d, mn_d, mx_d, order_d if with_order else None, ws_d, B, N, C, thr, thr_iou)
    torch.cuda.synchronize()
    assert guards_intact(conf_whole, B * N * C, CONF_GUARD), 'conf guards'
    assert guards_intact(ws_whole, ws_bytes // 4, WS_GUARD), 'ws guards'
    assert guards_intact(order_whole, B * N, ORDER_GUARD), 'order guards'
    if not with_order:
        assert bool((order_whole == ORDER_GUARD).all().item()), 'a buffer that was not passed'
    assert np.array_equal(M.bits(mn_d.cpu().numpy()), M.bits(mn)) and np.array_equal(M.bits(mx_d.cpu().numpy()), M.bits(mx)), 'boxes'
    got = conf_d.view(torch.int32).cpu().numpy().view(np.uint32).reshape(B, N, C)
    return got, (order_d.cpu().numpy().reshape(B, N) if with_order else None)


@pytest.mark.parametrize('name', ORDER)
def test_nms_case_vs_oracle(ops, name):
    c = M.case(name)
    ref_conf, ref_order = M.reference(name)
    stream = torch.cuda.Stream() if name == M.SIDE_STREAM_CASE else None
    args = (c['thr'], c['thr_iou'], c['with_order'])
    got, order = launch(ops, c['conf'], c['xy_min'], c['xy_max'], *args, stream=stream)
    ref_bits = M.bits(ref_conf)
    for b in range(c['B']):
        wrong = np.argwhere(got[b] != ref_bits[b])
        assert len(wrong) == 0, '%s image %d: %d scores differ, first (box, class) %s' % (name, b, len(wrong), wrong[:4].tolist())
        if c['with_order']:
            assert np.array_equal(order[b], ref_order[b]), '%s image %d: order differs at %s' % (name, b, np.flatnonzero(order[b] != ref_order[b])[:4])
    # the same call on fresh copies: the same bits (an LDS race would show as a difference)
    again, order2 = launch(ops, c['conf'], c['xy_min'], c['xy_max'], *args, stream=stream)
    assert np.array_equal(again, got) and (order is None or np.array_equal(order2, order))
    # every image alone equals its part of the batch
    for b in range(c['B']):
        one, order1 = launch(ops, c['conf'][b:b + 1], c['xy_min'][b:b + 1], c['xy_max'][b:b + 1], *args, stream=stream)
        assert np.array_equal(one[0], got[b]) and (order is None or np.array_equal(order1[0], order[b])), '%s image %d alone' % (name, b)


@pytest.mark.parametrize('B,N,C', [(1, 4097, 1), (1, 0, 3), (0, 64, 3), (2, 64, 0), (1, -1, 1)])
def test_nms_refuses_what_it_cannot_serve_and_writes_nothing(ops, B, N, C):
    """Refused on the host before any launch (csrc/nms.hip Y2_CHECK_ARG): HipKernelError, and no buffer is touched."""
    from yolo_tf_amd._lib import HipKernelError
    n = 4097 * 4
    conf_whole, conf_d = guarded(n, torch.float32, CONF_GUARD)
    order_whole, order_d = guarded(n, torch.int32, ORDER_GUARD)
    ws_whole, ws_d = guarded(n, torch.int32, WS_GUARD)
    rng = np.random.RandomState(7)
    boxes = rng.uniform(0, 5, (n, 2)).astype(np.float32)
    mn_d, mx_d = torch.from_numpy(boxes).cuda(), torch.from_numpy(boxes + np.float32(1)).cuda()
    scores = rng.uniform(0.5, 1, n).astype(np.float32)
    conf_d.copy_(torch.from_numpy(scores))
    torch.cuda.synchronize()
    with pytest.raises(HipKernelError):
        ops.nms(conf_d, mn_d, mx_d, order_d, ws_d, B, N, C, 0.3, 0.4)
    torch.cuda.synchronize()
    assert np.array_equal(M.bits(conf_d.cpu().numpy()), M.bits(scores))
    assert guards_intact(conf_whole, n, CONF_GUARD)
    assert bool((order_whole == ORDER_GUARD).all().item()) and bool((ws_whole == WS_GUARD).all().item())
    assert np.array_equal(mn_d.cpu().numpy(), boxes) and np.array_equal(mx_d.cpu().numpy(), boxes + np.float32(1))
