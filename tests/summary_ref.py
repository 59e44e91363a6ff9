"""Specification of the histogram summaries in NumPy f64 (the checker of csrc/summary.hip and yolo_tf_amd/summary.py).

Restates TensorFlow 1.x ``core/lib/histogram/histogram.cc`` as ``tf.summary.histogram`` uses it.  TensorFlow is not a dependency of
this project and the restatement has not been run against it (DESIGN.md says so): this file IS the contract.

    limits   v = 1e-12; while v < 1e20: pos.append(v); v *= 1.1        (repeated f64 multiplication: 774 values)
             [-p for p in reversed(pos)] + [0.0] + pos + [DBL_MAX]     (1550 limits = 1550 buckets)
    add(x)   finite x, widened exactly to f64 -> bucket upper_bound(limits, x); min, max, num, sum += x, sum_squares += x * x
             NaN / +-inf: left out of every statistic and counted in ``nonfinite`` (TensorFlow aborts the summary op instead)
    empty    min = DBL_MAX, max = -DBL_MAX, num = 0
    encode   EncodeToProto(preserve_zero_buckets = false): a run of empty buckets collapses into ONE entry carrying the run's last
             limit and count 0; every non-empty bucket is emitted with its own limit; nothing emitted -> (DBL_MAX, 0)
"""
import math

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)


def _limits():
    pos = []
    v = 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    return np.array([-p for p in reversed(pos)] + [0.0] + pos + [DBL_MAX], np.float64), np.array(pos, np.float64)


LIMITS, POS = _limits()
BUCKETS = len(LIMITS)


def bucket_of(x):
    """Bucket index of every (finite) element of ``x``."""
    return np.searchsorted(LIMITS, np.asarray(x, np.float64).reshape(-1), side='right')


def histogram(x):
    """x: any array of f32 / f64 values (bf16 callers widen first, which is exact).  Returns a dict: counts [1550] int64, min, max, sum,
    sum_squares (sums by math.fsum: correctly rounded), num, nonfinite, and abs_sum (the sum of |x|, for the tolerance on ``sum``)."""
    v = np.asarray(x).astype(np.float64).reshape(-1)
    fin = np.isfinite(v)
    f = v[fin]
    counts = np.bincount(bucket_of(f), minlength=BUCKETS).astype(np.int64)
    return {'counts': counts,
            'min': float(f.min()) if f.size else DBL_MAX,
            'max': float(f.max()) if f.size else -DBL_MAX,
            'sum': math.fsum(f),
            'sum_squares': math.fsum(f * f),          # squares of f32 / bf16 values are exact in f64
            'abs_sum': math.fsum(np.abs(f)),
            'num': int(f.size),
            'nonfinite': int(v.size - f.size)}


def sum_bounds(ref):
    """(bound on |sum - ref sum|, bound on |sum_squares - ref sum_squares|) for an f64 accumulation of ``num`` terms in ANY order:
    the classical (n - 1) u sum|x_i| with u = 2^-53, written n * 2^-52 * sum|x_i| -- a factor 2 of slack."""
    n = max(ref['num'], 1)
    return n * 2.0 ** -52 * ref['abs_sum'], n * 2.0 ** -52 * ref['sum_squares']


def encode_buckets(counts):
    """-> (bucket_limit list, bucket list) of HistogramProto, as EncodeToProto(proto, preserve_zero_buckets=false) emits them."""
    counts = np.asarray(counts)
    assert counts.shape == (BUCKETS,)
    limit, bucket = [], []
    i = 0
    while i < BUCKETS:
        c = float(counts[i])
        end = float(LIMITS[i])
        i += 1
        if c <= 0.0:
            while i < BUCKETS and counts[i] <= 0:      # the run of empties collapses; its LAST limit stays
                end = float(LIMITS[i])
                i += 1
        limit.append(end)
        bucket.append(c)
    if not any(bucket):
        # (every bucket empty: the walk above produced the single entry (DBL_MAX, 0), which is also what TensorFlow emits when nothing was)
        return [DBL_MAX], [0.0]
    return limit, bucket
