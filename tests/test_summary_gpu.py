"""yolo2_histogram (csrc/summary.hip) against the specification tests/summary_ref.py: counts, num, nonfinite, min and max exact; the f64 sums
within n * 2^-52 * sum|x| (resp. sum x^2) of math.fsum; every record bitwise the same whatever else is in the call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import summary_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _run(jobs):
    """jobs: [(tensor, rows, c, ld)] -> (raw int64 words [n][WORDS] as numpy, decoded dicts)."""
    torch = _torch()
    from yolo_tf_amd import ops
    h = ops.HistogramJobs(jobs)
    h.launch()
    torch.cuda.synchronize()
    words = h.out.cpu().numpy()
    return words, ops.decode_histograms(words)


def _widen(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _check(got, values, what=''):
    """One decoded record against the specification applied to the f64 array ``values``."""
    ref = S.histogram(values)
    assert got['num'] == ref['num'] and got['nonfinite'] == ref['nonfinite'], (what, got['num'], ref['num'], got['nonfinite'], ref['nonfinite'])
    bad = np.nonzero(got['counts'] != ref['counts'])[0]
    assert bad.size == 0, (what, bad[:8], got['counts'][bad[:8]], ref['counts'][bad[:8]])
    assert got['min'] == ref['min'] and got['max'] == ref['max'], (what, got['min'], ref['min'], got['max'], ref['max'])
    bs, bq = S.sum_bounds(ref)
    assert abs(got['sum'] - ref['sum']) <= bs, (what, got['sum'], ref['sum'], bs)
    assert abs(got['sum_squares'] - ref['sum_squares']) <= bq, (what, got['sum_squares'], ref['sum_squares'], bq)


def test_every_bf16_bit_pattern():
    torch = _torch()
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).cuda()
    x = bits.view(torch.bfloat16)
    words, (got,) = _run([(x, 1, 65536, 65536)])
    values = _widen(x)
    assert got['nonfinite'] == 2 * 127 + 2            # 127 NaN mantissas per sign and the two infinities
    _check(got, values, 'bf16')
    # value by value, not only in total: one job per 256-pattern page agrees with the page's own reference
    pages = [(x[i:i + 256], 1, 256, 256) for i in range(0, 65536, 256)]
    _, per_page = _run(pages)
    for i, g in enumerate(per_page):
        _check(g, values[i * 256:(i + 1) * 256], 'page %d' % i)


def test_f32_neighbours_of_every_limit():
    torch = _torch()
    finite = S.LIMITS[:-1]
    assert finite.size == 1549
    f = finite.astype(np.float32)
    vals = np.concatenate([f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf)),
                           np.array([0.0, -0.0, 1e-45, -1e-45, np.finfo(np.float32).max, -np.finfo(np.float32).max], np.float32)]).astype(np.float32)
    x = torch.from_numpy(vals).cuda()
    _, (got,) = _run([(x, 1, x.numel(), x.numel())])
    _check(got, vals.astype(np.float64), 'f32 limits')
    # one value per job: the bucket of each single value (the first 3 * 1549 + 6 jobs of one call)
    _, singles = _run([(x[i:i + 1], 1, 1, 1) for i in range(x.numel())])
    want = S.bucket_of(vals.astype(np.float64))
    for i, g in enumerate(singles):
        assert g['num'] == 1 and g['counts'][want[i]] == 1, (i, float(vals[i]), int(want[i]), np.nonzero(g['counts'])[0])


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4099, 16383, 16384, 16385, 40000]


def test_many_jobs_alone_together_and_reversed():
    torch = _torch()
    rng = np.random.RandomState(0)
    total = sum(SIZES[i % len(SIZES)] + 3 for i in range(200)) + 8
    pool32 = torch.from_numpy(rng.standard_normal(total).astype(np.float32)).cuda()
    pool16 = torch.from_numpy(rng.standard_normal(total).astype(np.float32)).cuda().to(torch.bfloat16)
    jobs, values = [], []
    off = 1
    for i in range(200):
        n = SIZES[i % len(SIZES)]
        scale = (1e-3, 1.0, 1e3)[i % 3]
        pool = pool16 if i % 2 else pool32
        view = pool[off:off + n]                      # bases at odd element offsets (every job advances by an even count)
        view.mul_(scale)
        jobs.append((view, 1 if n else 0, n, n))
        values.append(_widen(view))
        off += n + (2 if n % 2 == 0 else 3)
        assert off % 2 == 1
    words, got = _run(jobs)
    for i, (g, v) in enumerate(zip(got, values)):
        _check(g, v, 'job %d (n = %d)' % (i, v.size))
    words_again, _ = _run(jobs)
    assert np.array_equal(words, words_again)                         # two identical calls: the same bytes
    words_rev, _ = _run(jobs[::-1])
    assert np.array_equal(words, words_rev[::-1])                     # the list reversed
    for i in range(0, 200):                                           # each job submitted alone
        alone, _ = _run([jobs[i]])
        assert np.array_equal(alone[0], words[i]), i


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_strided_jobs_never_read_their_padding(dtype):
    torch = _torch()
    T = torch.bfloat16 if dtype == 'bf16' else torch.float32
    rng = np.random.RandomState(1)
    jobs, values = [], []
    for c, ld in [(1, 8), (3, 8), (5, 8), (8, 8), (125, 128), (13, 13), (5, 7)]:
        for rows in (1, 7, 338):
            a = rng.standard_normal((rows, ld)).astype(np.float32)
            if ld > c:
                a[:, c:] = np.where(np.arange(ld - c) % 2 == 0, np.nan, 1e30)[None, :]
            t = torch.from_numpy(a).cuda().to(T).contiguous()
            jobs.append((t, rows, c, ld))
            values.append(_widen(t)[:, :c].reshape(-1))
    _, got = _run(jobs)
    for (t, rows, c, ld), g, v in zip(jobs, got, values):
        assert g['nonfinite'] == 0 and g['num'] == rows * c, (rows, c, ld, g['nonfinite'], g['num'])
        _check(g, v, 'rows %d c %d ld %d' % (rows, c, ld))


def test_concentration_beyond_f32_exactness():
    """2^24 + 5 copies of one value: a counter kept in f32 would stop counting at 2^24."""
    torch = _torch()
    n = (1 << 24) + 5
    value = np.float32(0.0123)
    others = np.array([-7.5, 3e-9, 2.5e7, -0.0123, 1.0], np.float32)
    x = torch.full((n + others.size,), float(value), dtype=torch.float32, device='cuda')
    where = [0, 12345, 1 << 20, (1 << 24) - 1, n + others.size - 1]
    for w, o in zip(where, others):
        x[w] = float(o)
    _, (got,) = _run([(x, 1, x.numel(), x.numel())])
    want = np.zeros(S.BUCKETS, np.int64)
    want[S.bucket_of([float(value)])[0]] = n
    for o in others:
        want[S.bucket_of([float(o)])[0]] += 1
    assert got['num'] == n + others.size and got['nonfinite'] == 0
    assert np.array_equal(got['counts'], want), np.nonzero(got['counts'] != want)[0]
    assert got['min'] == -7.5 and got['max'] == 2.5e7
    import math
    v, o64 = float(value), others.astype(np.float64)
    ref_sum, ref_sq = math.fsum([n * v] + list(o64)), math.fsum([n * v * v] + list(o64 * o64))
    abs_sum = n * abs(v) + float(np.abs(o64).sum())
    m = n + others.size
    # (n * v and n * v * v are each one rounding away from the exact sums: 2 ulp of slack on top of the any-order bound)
    assert abs(got['sum'] - ref_sum) <= m * 2.0 ** -52 * abs_sum + 2 * np.spacing(ref_sum)
    assert abs(got['sum_squares'] - ref_sq) <= m * 2.0 ** -52 * ref_sq + 2 * np.spacing(ref_sq)


def test_bad_arguments_raise():
    torch = _torch()
    from yolo_tf_amd import _lib, ops
    x = torch.zeros(16, device='cuda')
    with pytest.raises(AssertionError):
        ops.HistogramJobs([(x, 2, 8, 16)])            # 24 elements on a tensor of 16
    with pytest.raises(_lib.HipKernelError, match='argument check failed'):
        _lib.call('yolo2_histogram', None, 1, 0, None, 0, None, 0, None)
