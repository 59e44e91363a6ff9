"""NumPy specification of the int8 calibration histograms and clipping thresholds (DESIGN.md section 15 "Calibration methods").  Test
infrastructure only: the product never imports it, and it imports nothing of the product.

Histogram of |x| over [0, limit] in BINS equal bins (what yolo2_calib_histogram computes, bit for bit).  For every element, in f32:
  a = |x|;  NaN or inf: counted as non-finite, in no bin
  t = a * inv_width, inv_width = float32(BINS) / limit          one multiply, one rounding
  b = BINS - 1 if t >= BINS else int(t)                          compare before converting
  a > limit: also counted as clamped (it sits in the last bin)

Thresholds, in f64, from a histogram h with w = limit / BINS; candidates T_i = i * w, i = FIRST .. BINS, the smallest i wins ties:
  percentile p   need = ceil(total * p / 100); b = first bin whose cumulative count reaches need; T = (b + 1) * w (no lower bound); p = 100: limit
  mse            x_b = (b + 0.5) w; s = T / 127; q_b = min(rint(x_b / s), 127) * s; minimise sum h_b (x_b - q_b)^2
  entropy        P = h[0:i] with sum(h[i:]) added to P[i - 1]; Q: bins 0 .. i-1 in 128 groups by b * 128 // i, each group's sum of h[0:i] spread
                 evenly over its non-zero bins; both normalised; KL = sum over P > 0 of P ln(P / Q); a candidate with Q = 0 where P > 0 is skipped
"""
import math

import numpy as np

F32 = np.float32
BINS = 2048
FIRST = 128


def inv_width(limit):
    return F32(F32(BINS) / F32(limit))


def abs_histogram(x, limit):
    """x: array (read as f32), limit: f32 > 0 -> (counts int64 [BINS], non-finite count, clamped count)"""
    limit = F32(limit)
    a = np.abs(np.asarray(x, F32).reshape(-1))
    finite = np.isfinite(a)
    a = a[finite]
    with np.errstate(over='ignore', invalid='ignore'):
        t = (a * inv_width(limit)).astype(F32)                   # may overflow to +inf: the comparison comes first
        b = np.where(t >= F32(BINS), np.int64(BINS - 1), np.minimum(t, F32(BINS)).astype(np.int64))
    return np.bincount(b, minlength=BINS).astype(np.int64), int((~finite).sum()), int((a > limit).sum())


def percentile_threshold(h, limit, p):
    total = int(sum(int(v) for v in h))
    if p >= 100 or total == 0:
        return float(limit)
    need = int(math.ceil(total * float(p) / 100.0))
    w = float(limit) / BINS
    run = 0
    for b in range(BINS):
        run += int(h[b])
        if run >= need:
            return (b + 1) * w
    return float(limit)


def mse_objective(h, limit, i):
    """One candidate: a vector over the bins, summed exactly (math.fsum)."""
    w = float(limit) / BINS
    s = i * w / 127.0
    x = (np.arange(BINS, dtype=np.float64) + 0.5) * w
    q = np.minimum(np.rint(x / s), 127.0) * s
    return math.fsum(np.asarray(h, np.float64) * (x - q) ** 2)


def kl_objective(h, limit, i):
    """-> KL of candidate i, or None if it is skipped"""
    h = np.asarray(h, np.float64)
    P = h[:i].copy()
    P[i - 1] += math.fsum(h[i:])
    Q = np.zeros(i)
    for g in range(128):
        lo, hi = -(-g * i // 128), -(-(g + 1) * i // 128)          # the bins with b * 128 // i == g: a run, ceil(g i / 128) <= b < ceil((g + 1) i / 128)
        part = h[lo:hi]
        n = int((part > 0).sum())
        if n:
            Q[lo:hi] = np.where(part > 0, math.fsum(part) / n, 0.0)
    pos = P > 0
    if (Q[pos] == 0).any():
        return None
    P, Q = P / math.fsum(P), Q / math.fsum(Q)
    return math.fsum(P[pos] * np.log(P[pos] / Q[pos]))


def objectives(h, limit, method):
    """-> {i: objective} over the candidates that are not skipped"""
    f = {'mse': mse_objective, 'entropy': kl_objective}[method]
    out = {}
    for i in range(FIRST, BINS + 1):
        v = f(h, limit, i)
        if v is not None:
            out[i] = v
    return out


def best_candidate(obj):
    best = None
    for i in sorted(obj):
        if best is None or obj[i] < obj[best]:
            best = i
    return best


def threshold(h, limit, method, p=99.99):
    if method == 'percentile':
        return percentile_threshold(h, limit, p)
    if int(np.asarray(h).sum()) == 0:
        return float(limit)
    i = best_candidate(objectives(h, limit, method))
    return (BINS if i is None else i) * (float(limit) / BINS)
