"""yolo2_image_summary (csrc/image_summary.hip) against the specification tests/image_summary_ref.py: every byte, image_min, image_max,
scale and the count of non-finite pixels equal, no tolerance anywhere; the same bytes whether a job runs alone, among the others or with
the list reversed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_summary_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAN, INF = np.nan, np.inf


def _torch():
    import torch
    return torch


def _run(jobs):
    """jobs: [(tensor, rows, c, ld)] -> (the raw result buffer as numpy, [(record, uint8 [rows][depth])])."""
    torch = _torch()
    from yolo_tf_amd import ops
    t = ops.ImageJobs(jobs)
    t.launch()
    torch.cuda.synchronize()
    buf = t.out.cpu().numpy()
    return buf, ops.decode_images(buf, t.shapes, t.offsets)


def _check(got, values, what=''):
    """One decoded job against the specification applied to ``values`` [rows][c] f32 (the job's own values, padding stripped)."""
    rec, pix = got
    rows, c = values.shape
    if rows == 0:
        assert pix.size == 0 and rec['min'] == INF and rec['max'] == -INF and rec['nonfinite'] == 0 and rec['scale'] == 0.0, (what, rec)
        return
    x = values.reshape(1, rows, c)
    if c not in (1, 3, 4):
        x = R.channel_sum(x)[..., None]
    want, info = R.normalize_image(x)
    print('%s: rows %d c %d min %r max %r scale %r nonfinite %d' % (what, rows, c, rec['min'], rec['max'], rec['scale'], rec['nonfinite']))
    assert rec['nonfinite'] == info['nonfinite'], (what, rec, info)
    assert rec['min'] == info['min'] and rec['max'] == info['max'], (what, rec, info)
    assert np.float32(rec['scale']).tobytes() == np.float32(info['scale']).tobytes(), (what, rec, info)
    want = want.reshape(rows, -1)
    bad = np.nonzero(pix != want)
    assert bad[0].size == 0, (what, bad[0][:8], bad[1][:8], pix[bad][:8], want[bad][:8])


def _device(a, dtype, ld=None, poison=True, odd_base=False):
    """a: [rows][c] f32 -> (device tensor whose data_ptr() is the job's base, ld, the values as the device holds them [rows][c] f32).
    ld > c: the padding lanes hold NaN and 1e30 alternately.  odd_base: the job starts one element into its allocation."""
    torch = _torch()
    T = torch.bfloat16 if dtype == 'bf16' else torch.float32
    rows, c = a.shape
    ld = c if ld is None else ld
    full = np.zeros((rows, ld), np.float32)
    full[:, :c] = a
    if ld > c and poison:
        full[:, c:] = np.where(np.arange(ld - c) % 2 == 0, NAN, 1e30)[None, :]
    flat = np.concatenate([np.full(1 if odd_base else 0, NAN, np.float32), full.reshape(-1)])
    t = torch.from_numpy(flat).cuda().to(T).contiguous()
    view = t[1:] if odd_base else t
    held = view.float().cpu().numpy()[:rows * ld].reshape(rows, ld)[:, :c].copy()
    return view, ld, held


def _classes(rng, rows, c):
    """The value classes of the specification, each [rows][c]: all zero, non-negative, mixed sign, some NaN / +-inf pixels, all non-finite,
    below the 1e-6 threshold."""
    pos = np.abs(rng.standard_normal((rows, c))).astype(np.float32) * 3
    mixed = rng.standard_normal((rows, c)).astype(np.float32)
    holes = mixed.copy() * 5
    flat = holes.reshape(-1)
    flat[rng.permutation(flat.size)[:max(1, flat.size // 7)]] = np.array([NAN, INF, -INF], np.float32)[rng.randint(0, 3, max(1, flat.size // 7))]
    nothing = np.full((rows, c), NAN, np.float32)
    nothing.reshape(-1)[::2] = INF
    tiny = (rng.rand(rows, c).astype(np.float32) - 0.3) * np.float32(1e-7)
    return [('zero', np.zeros((rows, c), np.float32)), ('non-negative', pos), ('mixed', mixed), ('holes', holes), ('all non-finite', nothing), ('tiny', tiny)]


def _cases():
    """Every job of the issue's table: (what, values [rows][c], dtype, ld, odd_base)."""
    rng = np.random.RandomState(0)
    cases = [('f32 5x7x3', rng.standard_normal((35, 3)).astype(np.float32), 'f32', 3, False),
             ('bf16 13x13x40 in 48, poisoned padding', rng.standard_normal((169, 40)).astype(np.float32), 'bf16', 48, False),
             ('bf16 2x2x1024', rng.standard_normal((4, 1024)).astype(np.float32) * 2, 'bf16', 1024, False),
             ('bf16 104x104x64: more than one workgroup', rng.standard_normal((104 * 104, 64)).astype(np.float32), 'bf16', 64, False),
             ('bf16 one pixel', rng.standard_normal((1, 1)).astype(np.float32), 'bf16', 1, False),
             ('bf16 one pixel of 24 channels', rng.standard_normal((1, 24)).astype(np.float32), 'bf16', 24, False),
             ('bf16 empty', np.zeros((0, 8), np.float32), 'bf16', 8, False)]
    sizes = [(16, 16), (15, 16), (3, 5), (1, 2)]
    k = 0
    for dtype in ('f32', 'bf16'):
        for c in (1, 4, 2):
            for what, a in _classes(rng, sizes[k % len(sizes)][0] * sizes[k % len(sizes)][1], c):
                cases.append(('%s c=%d %s' % (dtype, c, what), a, dtype, c, False))
                k += 1
    # summed jobs of the value classes (a non-finite channel makes the pixel's sum non-finite), vector and scalar load paths
    for dtype in ('f32', 'bf16'):
        for what, a in _classes(rng, 7 * 9, 24):
            cases.append(('%s c=24 %s' % (dtype, what), a, dtype, 24, False))
        cases.append(('%s c=13 ld=13 (odd stride)' % dtype, rng.standard_normal((50, 13)).astype(np.float32), dtype, 13, False))
        cases.append(('%s c=40 odd base' % dtype, rng.standard_normal((50, 40)).astype(np.float32), dtype, 48, True))
        cases.append(('%s c=3 odd base' % dtype, rng.standard_normal((50, 3)).astype(np.float32), dtype, 3, True))
        cases.append(('%s c=3 in 8' % dtype, rng.standard_normal((50, 3)).astype(np.float32) * 100, dtype, 8, False))
    # a channel sum whose f64 result is not exact, mixed magnitudes: another order gives another f32
    # (small values around a pair +A, -A of about 2^30 .. 2^60 at random channels: which small terms are absorbed depends on where the
    # chain stands when it meets them, and what survives is what is left after the pair cancels)
    mag = (rng.standard_normal((64, 72)) * np.exp2(rng.randint(-8, 8, (64, 72)))).astype(np.float32)
    for p in range(64):
        i, j = rng.permutation(72)[:2]
        mag[p, i] = np.float32((1 + rng.rand()) * 2.0 ** rng.randint(30, 60))
        mag[p, j] = -mag[p, i]
    cases.append(('f32 c=72 mixed magnitudes', mag, 'f32', 72, False))
    cases.append(('bf16 c=72 mixed magnitudes', mag, 'bf16', 80, False))
    return cases


_SHARED = {}


def _shared():
    """The jobs of _cases() on the device and the result of running them all in one call: computed once, read by several tests."""
    if not _SHARED:
        jobs, values, names = [], [], []
        for what, a, dtype, ld, odd in _cases():
            view, ld, held = _device(a, dtype, ld, odd_base=odd)
            jobs.append((view, a.shape[0], a.shape[1], ld))
            values.append(held)
            names.append(what)
        buf, got = _run(jobs)
        _SHARED.update(jobs=jobs, values=values, names=names, buf=buf, got=got)
    return _SHARED


def test_every_case_equals_the_specification_bitwise():
    s = _shared()
    assert any(j[0].data_ptr() % 4 == 2 for j in s['jobs']) and any(j[0].data_ptr() % 16 == 4 for j in s['jobs'])     # odd bases, bf16 and f32
    for what, g, v in zip(s['names'], s['got'], s['values']):
        _check(g, v, what)


def test_mixed_magnitude_sum_depends_on_the_order():
    """The mixed-magnitude case is one where the order of the additions shows: plain left-to-right f64 summation and f32 accumulation
    both differ from the specification's order somewhere -- so the kernel, which is bitwise the specification, follows that order."""
    s = _shared()
    v = s['values'][s['names'].index('f32 c=72 mixed magnitudes')]
    spec = R.channel_sum(v)
    seq = np.zeros(v.shape[0], np.float64)
    for j in range(v.shape[1]):
        seq = seq + v[:, j].astype(np.float64)
    assert np.any(seq.astype(np.float32) != spec) and np.any(v.astype(np.float64).sum(-1).astype(np.float32) != spec)
    for what in ('f32 c=72 mixed magnitudes', 'bf16 c=72 mixed magnitudes'):
        v = s['values'][s['names'].index(what)]
        assert np.any(np.cumsum(v, -1, dtype=np.float32)[:, -1] != R.channel_sum(v)), what


def test_alone_together_and_reversed_give_the_same_bytes():
    from yolo_tf_amd import ops
    s = _shared()
    jobs, got = s['jobs'], s['got']
    _, again = _run(jobs)
    _, rev = _run(jobs[::-1])
    rev = rev[::-1]
    n = ops.IMAGE_RECORD_BYTES
    for i, what in enumerate(s['names']):
        for other in (again[i], rev[i], _run([jobs[i]])[1][0]):
            assert np.array_equal(other[1], got[i][1]), what
            assert np.float32([other[0][k] for k in ('min', 'max', 'scale')]).tobytes() == np.float32([got[i][0][k] for k in ('min', 'max', 'scale')]).tobytes(), what
            assert other[0]['nonfinite'] == got[i][0]['nonfinite'], what
    assert n == 16


def test_padding_and_neighbours_never_reach_the_result():
    """The same values with clean and with poisoned padding lanes: identical results (and no non-finite pixel reported)."""
    rng = np.random.RandomState(5)
    for dtype in ('bf16', 'f32'):
        for c, ld in ((40, 48), (3, 8), (1, 2), (5, 7), (125, 128)):
            a = rng.standard_normal((30, c)).astype(np.float32)
            v1, _, held = _device(a, dtype, ld, poison=True)
            v2, _, _ = _device(a, dtype, ld, poison=False)
            _, (g1, g2) = _run([(v1, 30, c, ld), (v2, 30, c, ld)])
            assert g1[0]['nonfinite'] == 0 and np.array_equal(g1[1], g2[1]) and g1[0] == g2[0], (dtype, c, ld)
            _check(g1, held, '%s c=%d ld=%d' % (dtype, c, ld))


def test_output_beyond_a_job_is_left_alone():
    """Jobs write rows * depth bytes at their offsets and nothing else: the gaps of the 16-byte aligned layout keep the zeros they had."""
    from yolo_tf_amd import ops
    s = _shared()
    t = ops.ImageJobs(s['jobs'])
    used = np.zeros(t.out.numel(), bool)
    used[:t.n * ops.IMAGE_RECORD_BYTES] = True
    for (rows, depth), off in zip(t.shapes, t.offsets):
        used[off:off + rows * depth] = True
    assert not s['buf'][~used].any() and (~used).sum() > 0


def test_bad_arguments_raise():
    torch = _torch()
    from yolo_tf_amd import _lib, ops
    x = torch.zeros(16, device='cuda')
    with pytest.raises(AssertionError):
        ops.ImageJobs([(x, 2, 8, 16)])                # 24 elements on a tensor of 16
    with pytest.raises(AssertionError):
        ops.ImageJobs([(x, 2, 9, 8)])                 # c > ld
    with pytest.raises(ValueError):
        ops.ImageJobs([(x.to(torch.float16), 2, 8, 8)])
    with pytest.raises(_lib.HipKernelError, match='argument check failed'):
        _lib.call('yolo2_image_summary', None, 1, 0, None, 0, None, 0, None)
    t = ops.ImageJobs([(x, 2, 8, 8)])
    with pytest.raises(_lib.HipKernelError, match='argument check failed'):      # a result buffer smaller than the records
        _lib.call('yolo2_image_summary', ops.ptr(t.table), 1, t.items, ops.ptr(t.out), 8, ops.ptr(t.ws), t.ws.numel() * 4, None)
    with pytest.raises(_lib.HipKernelError, match='argument check failed'):      # a misaligned result buffer
        _lib.call('yolo2_image_summary', ops.ptr(t.table), 1, t.items, ops.ptr(t.out) + 1, t.out.numel() - 1, ops.ptr(t.ws), t.ws.numel() * 4, None)
