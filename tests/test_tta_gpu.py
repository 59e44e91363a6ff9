"""yolo2_wbf and yolo2_tta_gather (csrc/tta.hip) against their specification (tests/tta_ref.py) on the cases of tests/tta_cases.py: scores and
boxes as uint32 bit patterns (the zeroed tail is +0.0, not -0.0), rows and flags as integers.  Every output is a slice of a larger buffer with
64 sentinel elements on either side, and the workspace starts with arbitrary content.  What each case exercises, and the proof that a subtly
wrong fusion differs on some of them, is in tests/test_tta_cpu.py.

The order of ORDER matters: the case with YOLO2_WBF_MAX_CANDIDATES candidates (the largest LDS request) comes between small ones, so that the
per-device bookkeeping of the raised LDS limit sees growing and shrinking requests."""
import numpy as np
import pytest
import torch

import tta_cases as M
import tta_ref as T

pytestmark = pytest.mark.gpu

GUARD = 64
F32_GUARD, INT_GUARD = 0x7FC0BEEF, -0x0BADBEEF
E_ARG = r'failed \(code 1\): .*argument check failed'      # YOLO2_E_ARG and the check's own message: not a launch failure (code 2)
_BIG = ['max_candidates', 'max_candidates_plus1']
ORDER = [n for n in M.NAMES if n not in _BIG][:20] + _BIG + [n for n in M.NAMES if n not in _BIG][20:]
assert sorted(ORDER) == sorted(M.NAMES)


@pytest.fixture(scope='module')
def ops():
    from yolo_tf_amd import ops as _ops
    _ops._lib.load()
    assert _ops.WBF_MAX_CANDIDATES == T.MAX_CANDIDATES
    assert (_ops.WBF_FLAG_CANDIDATES, _ops.WBF_FLAG_CLUSTERS, _ops.WBF_FLAG_ROWS) == (T.FLAG_CANDIDATES, T.FLAG_CLUSTERS, T.FLAG_ROWS)
    return _ops


def guarded(n, dtype, fill):
    """(whole buffer, the n elements between the guards)."""
    whole = torch.full((GUARD + n + GUARD,), fill, dtype=torch.int32, device='cuda')
    return whole, whole[GUARD:GUARD + n].view(dtype)


def guards_intact(whole, n, fill):
    return bool((whole[:GUARD] == fill).all().item()) and bool((whole[GUARD + n:] == fill).all().item())


def upload_bits(a):
    """f32 NumPy array -> device f32 tensor with the same bits (as integers: NaN payloads stay)."""
    return torch.from_numpy(M.bits(a).view(np.int32).copy()).cuda().view(torch.float32)


def launch(ops, conf, mn, mx, thr, fuse_iou, V, P, R, stream=None):
    """One call of ops.wbf on fresh guarded outputs: (out_conf bits [B,R,C], out_xy_min bits, out_xy_max bits [B,R,2], rows [B], flags)."""
    B, Mn, C = conf.shape
    outs = [guarded(B * R * k, torch.float32, F32_GUARD) for k in (C, 2, 2)]
    rows_whole, rows_d = guarded(B, torch.int32, INT_GUARD)
    flags_whole, flags_d = guarded(1, torch.int32, INT_GUARD)
    flags_d.zero_()
    ws = torch.full((ops.workspace_bytes('wbf', B, C, P),), 0x7F, dtype=torch.uint8, device='cuda')
    conf_d, mn_d, mx_d = upload_bits(conf), upload_bits(mn), upload_bits(mx)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        ops.wbf(conf_d, mn_d, mx_d, outs[0][1], outs[1][1], outs[2][1], rows_d, flags_d, ws, B, Mn, C, V, P, R, thr, fuse_iou)
    torch.cuda.synchronize()
    for (whole, _), k in zip(outs, (C, 2, 2)):
        assert guards_intact(whole, B * R * k, F32_GUARD), 'output guards'
    assert guards_intact(rows_whole, B, INT_GUARD) and guards_intact(flags_whole, 1, INT_GUARD), 'rows / flags guards'
    for d, a in ((conf_d, conf), (mn_d, mn), (mx_d, mx)):
        assert np.array_equal(M.bits(d.cpu().numpy()), M.bits(a)), 'an input was written'
    got = [o[1].view(torch.int32).cpu().numpy().view(np.uint32).reshape(B, R, k) for o, k in zip(outs, (C, 2, 2))]
    return got[0], got[1], got[2], rows_d.cpu().numpy(), int(flags_d.item())


def check(got, ref, what):
    oc, omn, omx, rows, flags = got
    assert flags == ref[4], '%s: flags %d, want %d' % (what, flags, ref[4])
    assert rows.tolist() == ref[3].tolist(), '%s: rows %s, want %s' % (what, rows.tolist(), ref[3].tolist())
    for name, g, r in (('out_conf', oc, ref[0]), ('out_xy_min', omn, ref[1]), ('out_xy_max', omx, ref[2])):
        wrong = np.argwhere(g != M.bits(r))
        assert len(wrong) == 0, '%s %s: %d values differ, first %s: got %s, want %s' % (
            what, name, len(wrong), wrong[:4].tolist(), [hex(g[tuple(w)]) for w in wrong[:4]], [hex(M.bits(r)[tuple(w)]) for w in wrong[:4]])
    for b in range(len(rows)):                               # the tail: +0.0 everywhere
        assert not oc[b, rows[b]:].any() and not omn[b, rows[b]:].any() and not omx[b, rows[b]:].any(), '%s: tail of image %d' % (what, b)


@pytest.mark.parametrize('name', ORDER)
def test_wbf_case_vs_specification(ops, name):
    c = M.case(name)
    args = (c['thr'], c['fuse_iou'], c['V'], c['max_per_class'], c['R'])
    got = launch(ops, c['conf'], c['xy_min'], c['xy_max'], *args)
    check(got, M.reference(name), name)
    if c['M'] <= 1024:
        # the same call on fresh buffers: the same bits (an LDS race would show as a difference)
        again = launch(ops, c['conf'], c['xy_min'], c['xy_max'], *args, stream=torch.cuda.Stream() if name == 'c3_b3_v2' else None)
        assert all(np.array_equal(a, g) for a, g in zip(again[:4], got[:4])) and again[4] == got[4]
    if c['B'] > 1 and M.reference(name)[4] == 0:
        # the last image alone equals its part of the batch
        b = c['B'] - 1
        one = launch(ops, c['conf'][b:b + 1], c['xy_min'][b:b + 1], c['xy_max'][b:b + 1], *args)
        assert all(np.array_equal(o[0], g[b]) for o, g in zip(one[:4], got[:4])), '%s image %d alone' % (name, b)


def test_flags_are_only_ored(ops):
    """A word that already holds a bit keeps it."""
    c = M.case('hand2')
    B, Mn, C = c['conf'].shape
    R = c['R']
    out = [torch.zeros(B * R * k, device='cuda') for k in (C, 2, 2)]
    rows, flags = torch.zeros(B, dtype=torch.int32, device='cuda'), torch.full((1,), 8, dtype=torch.int32, device='cuda')
    ws = torch.zeros(ops.workspace_bytes('wbf', B, C, 8), dtype=torch.uint8, device='cuda')
    ops.wbf(upload_bits(c['conf']), upload_bits(c['xy_min']), upload_bits(c['xy_max']), *out, rows, flags, ws, B, Mn, C, 2, 8, R, c['thr'], c['fuse_iou'])
    assert int(flags.item()) == 8 and rows.tolist() == [1]


def test_gather_two_views_at_offsets(ops):
    """B = 3, a view of 20 boxes and a flipped view of 45 boxes at another grid into a pooled buffer of 80 rows: rows 65 .. 79 are untouched."""
    rng = np.random.RandomState(11)
    B, C, Mn, w0, h0 = 3, 4, 80, 2, 2
    views = []
    for n, cw, ch, flip in ((20, 2, 2, False), (45, 3, 3, True), (20, 2, 2, True), (45, 3, 3, False)):
        mn = rng.uniform(0, cw - 1, (B, n, 2)).astype(np.float32)
        mx = (mn + rng.uniform(0, 1, (B, n, 2))).astype(np.float32)
        views.append((rng.uniform(0, 1, (B, n, C)).astype(np.float32), mn, mx, cw, ch, flip))
    for pair in (views[:2], views[2:]):
        pooled = [guarded(B * Mn * k, torch.float32, F32_GUARD) for k in (C, 2, 2)]
        before = [torch.from_numpy(rng.randint(0, 2 ** 31, B * Mn * k).astype(np.int32)).cuda() for k in (C, 2, 2)]
        for (_, p), s in zip(pooled, before):
            p.view(torch.int32).copy_(s)
        offset = 0
        for conf, mn, mx, cw, ch, flip in pair:
            sx, sy = T.scales(w0, h0, cw, ch)
            ops.tta_gather(upload_bits(conf), upload_bits(mn), upload_bits(mx), pooled[0][1], pooled[1][1], pooled[2][1], B, conf.shape[1], C, Mn, offset,
                           sx, sy, w0, flip)
            offset += conf.shape[1]
        torch.cuda.synchronize()
        want = T.gather(pair, w0, h0)
        for (whole, p), s, w, k in zip(pooled, before, want, (C, 2, 2)):
            assert guards_intact(whole, B * Mn * k, F32_GUARD)
            got = p.view(torch.int32).cpu().numpy().view(np.uint32).reshape(B, Mn, k)
            assert np.array_equal(got[:, :65], M.bits(w))
            assert np.array_equal(got[:, 65:], s.cpu().numpy().view(np.uint32).reshape(B, Mn, k)[:, 65:]), 'rows outside the views were written'


def test_gather_flip_twice_on_device(ops):
    rng = np.random.RandomState(12)
    B, n, C, w0 = 2, 70, 3, 13
    x = np.sort(rng.randint(0, 8 * w0 + 1, (B, n, 2)) / 8.0, axis=2).astype(np.float32)
    y = np.sort(rng.randint(0, 8 * w0 + 1, (B, n, 2)) / 8.0, axis=2).astype(np.float32)
    mn, mx = np.stack([x[..., 0], y[..., 0]], -1), np.stack([x[..., 1], y[..., 1]], -1)
    conf = rng.uniform(0, 1, (B, n, C)).astype(np.float32)
    a = [upload_bits(conf), upload_bits(mn), upload_bits(mx)]
    b = [torch.zeros_like(t) for t in a]
    c = [torch.zeros_like(t) for t in a]
    ops.tta_gather(*a, *b, B, n, C, n, 0, 1.0, 1.0, w0, True)
    ops.tta_gather(*b, *c, B, n, C, n, 0, 1.0, 1.0, w0, True)
    torch.cuda.synchronize()
    assert np.array_equal(b[1].cpu().numpy()[..., 0], np.float32(w0) - mx[..., 0])
    for got, want in zip(c, (conf, mn, mx)):
        assert np.array_equal(M.bits(got.cpu().numpy()), M.bits(want))


WBF_BAD = [dict(M=0), dict(M=32769), dict(C=0), dict(B=0), dict(thr=-1.0), dict(thr=float('nan')), dict(fuse_iou=float('inf')), dict(fuse_iou=float('nan')),
           dict(V=0), dict(P=0), dict(P=1025), dict(R=0)]


@pytest.mark.parametrize('bad', WBF_BAD, ids=lambda d: '%s=%s' % next(iter(d.items())))
def test_wbf_refuses_what_it_cannot_serve_and_writes_nothing(ops, bad):
    from yolo_tf_amd._lib import HipKernelError
    a = dict(dict(B=1, M=64, C=2, thr=0.1, fuse_iou=0.55, V=2, P=16, R=8), **bad)
    n = 64 * 2
    rng = np.random.RandomState(7)
    boxes = torch.from_numpy(rng.uniform(0, 5, (n, 2)).astype(np.float32)).cuda()
    conf = torch.from_numpy(rng.uniform(0.5, 1, n).astype(np.float32)).cuda()
    outs = [guarded(64, torch.float32, F32_GUARD) for _ in range(3)]
    rows_whole, rows_d = guarded(1, torch.int32, INT_GUARD)
    flags_whole, flags_d = guarded(1, torch.int32, INT_GUARD)
    ws = torch.full((ops.workspace_bytes('wbf', 1, 2, 16),), 0x7F, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    with pytest.raises(HipKernelError, match=E_ARG):
        ops.wbf(conf, boxes, boxes + 1, outs[0][1], outs[1][1], outs[2][1], rows_d, flags_d, ws, a['B'], a['M'], a['C'], a['V'], a['P'], a['R'], a['thr'],
                a['fuse_iou'])
    torch.cuda.synchronize()
    for whole in [o[0] for o in outs]:
        assert bool((whole == F32_GUARD).all().item())
    assert bool((rows_whole == INT_GUARD).all().item()) and bool((flags_whole == INT_GUARD).all().item()) and bool((ws == 0x7F).all().item())


GATHER_BAD = [dict(N=0), dict(M=0), dict(M=32769), dict(C=0), dict(B=0), dict(offset=-1), dict(offset=49), dict(sx=float('inf')), dict(sy=float('nan')),
              dict(w0=float('inf')), dict(flip=2)]


@pytest.mark.parametrize('bad', GATHER_BAD, ids=lambda d: '%s=%s' % next(iter(d.items())))
def test_gather_refuses_what_it_cannot_serve_and_writes_nothing(ops, bad):
    from yolo_tf_amd._lib import HipKernelError, call, ptr
    a = dict(dict(B=1, N=16, C=2, M=64, offset=48, sx=1.0, sy=1.0, w0=13.0, flip=0), **bad)
    src = [torch.ones(16 * k, device='cuda') for k in (2, 2, 2)]
    outs = [guarded(64 * 2, torch.float32, F32_GUARD) for _ in range(3)]
    torch.cuda.synchronize()
    with pytest.raises(HipKernelError, match=E_ARG):
        call('yolo2_tta_gather', ptr(src[0]), ptr(src[1]), ptr(src[2]), ptr(outs[0][1]), ptr(outs[1][1]), ptr(outs[2][1]), a['B'], a['N'], a['C'], a['M'],
             a['offset'], a['sx'], a['sy'], a['w0'], a['flip'], None)
    torch.cuda.synchronize()
    for whole in [o[0] for o in outs]:
        assert bool((whole == F32_GUARD).all().item())


def test_workspace_bytes(ops):
    assert ops.workspace_bytes('wbf', 3, 20, 256) >= 3 * 20 * (4 + 256 * 20)
    assert ops.workspace_bytes('wbf', 0, 20, 256) == 0
