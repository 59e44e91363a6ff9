"""The specification of yolo2_soft_nms (csrc/soft_nms.hip) in NumPy float32, `soft_exp` (csrc/soft_exp.h) included.  Every operation
is an IEEE f32 operation on np.float32 values, one rounding each, in the kernel's order, so the kernel's results equal these bit for bit.

Per (image b, class c), independently:

    s    = conf[b, :, c]
    cand = { i : s[i] > threshold }          # NaN and anything <= threshold is no candidate
    live = cand ; kept = {}
    while live is not empty:
        m = the element of live that is first by (s descending, box index ascending)
        if not (s[m] > threshold): break
        live -= {m} ; kept += {m}             # s[m] is final from here on
        for j in live:
            iou  = inter / max((a1 + a2) - inter, 1e-10f)       # csrc/nms.hip's operation order
            w    = hard:     iou >= threshold_iou ? 0 : 1
                   linear:   iou >= threshold_iou ? 1 - iou : 1
                   gaussian: soft_exp(-((iou * iou) / sigma))
            s[j] = s[j] * w
    write back: kept -> their s ; cand \\ kept -> +0.0f ; every non-candidate: bits untouched

order[b] = the box indices by (max over classes of the FINAL scores descending, box index ascending).

Boxes are finite with xy_min <= xy_max; scores are free of NaN where an order is asked for."""
import numpy as np

F = np.float32
METHODS = ('hard', 'linear', 'gaussian')
N_LIMIT = 4096
SIGMA_MIN = 1.0 / 64

LOG2E, LN2_HI, LN2_LO = F(1.44269504), F(0.693359375), F(-2.12194440e-4)
# 1/5040, 1/720, 1/120, 1/24, 1/6, 1/2, 1, 1: the degree-7 Taylor polynomial, highest coefficient first
POLY = (F(1.98412698e-4), F(1.38888889e-3), F(8.33333333e-3), F(4.16666667e-2), F(1.66666667e-1), F(0.5), F(1.0), F(1.0))


def soft_exp(x):
    """csrc/soft_exp.h operation for operation; x: f32 array in [-65, 0]."""
    x = np.asarray(x, F)
    n = np.rint(x * LOG2E)
    r = x - n * LN2_HI
    r = r - n * LN2_LO
    p = np.full(x.shape, POLY[0], F)
    for coef in POLY[1:]:
        p = p * r + coef
    scale = ((n.astype(np.int32) + np.int32(127)) << np.int32(23)).astype(np.uint32).view(F)
    out = p * scale
    assert out.dtype == F
    return out


def iou_with(mn, mx, area, m, js):
    """IoU of box m with the boxes js, in csrc/nms.hip's operation order."""
    w = np.maximum(np.minimum(mx[m, 0], mx[js, 0]) - np.maximum(mn[m, 0], mn[js, 0]), F(0))
    h = np.maximum(np.minimum(mx[m, 1], mx[js, 1]) - np.maximum(mn[m, 1], mn[js, 1]), F(0))
    inter = w * h
    return inter / np.maximum((area[m] + area[js]) - inter, F(1e-10))


def weight(iou, method, thr_iou, sigma):
    if method == 'hard':
        return np.where(iou >= thr_iou, F(0), F(1)).astype(F)
    if method == 'linear':
        return np.where(iou >= thr_iou, F(1) - iou, F(1)).astype(F)
    return soft_exp(-((iou * iou) / sigma))


def check_args(N, method, threshold, threshold_iou, sigma):
    assert method in METHODS and 1 <= N <= N_LIMIT
    assert threshold >= 0 and np.isfinite(threshold_iou)
    assert method != 'gaussian' or (np.isfinite(sigma) and sigma >= SIGMA_MIN)


def soft_nms_column(s, mn, mx, area, threshold, threshold_iou, method, sigma, stats=None):
    """One (image, class): s [N] f32 is updated in place.  stats, if a dict, receives what the pick loop went through."""
    thr, thr_iou, sigma = F(threshold), F(threshold_iou), F(sigma)
    live = np.flatnonzero(s > thr)                     # ascending box index
    K = len(live)
    cur = s[live].copy()
    final = np.zeros(K, F)                             # cand \ kept -> +0.0
    pos = np.arange(K)
    alive = np.ones(K, bool)
    picks = decay_ties = 0
    subnormal = floor = False
    tiny = np.finfo(F).tiny
    while alive.any():
        idx = pos[alive]
        k = idx[np.argmax(cur[idx])]                   # the first maximum = the lowest box index among equals
        if not (cur[k] > thr):
            break
        alive[k] = False
        final[k] = cur[k]
        picks += 1
        idx = pos[alive]
        if len(idx) == 0:
            break
        iou = iou_with(mn, mx, area, live[k], live[idx])
        before = cur[idx]
        cur[idx] = before * weight(iou, method, thr_iou, sigma)
        if stats is not None:
            after = cur[idx]
            subnormal = subnormal or bool(((after > 0) & (after < tiny)).any())
            floor = floor or bool(((area[live[k]] + area[live[idx]]) <= F(1e-10)).any())      # both areas zero: the union is the 1e-10 floor
            top = after[after > thr]
            if len(top) > 1:
                best = top.max()
                tied = idx[(after == best)]
                if len(tied) > 1 and len(np.unique(s[live[tied]])) > 1:
                    decay_ties += 1                    # equal now, different at the start: a tie the decay made
    if stats is not None:
        stats.update(K=K, picks=picks, zeroed=K - picks, decay_ties=decay_ties, subnormal=subnormal, floor=floor)
    s[live] = final
    return s


def soft_nms(conf, xy_min, xy_max, threshold, threshold_iou, method='gaussian', sigma=0.5, with_order=True, stats=None):
    """conf [B,N,C], xy_min / xy_max [B,N,2] f32 -> (new conf [B,N,C], order [B,N] int64 or None).  The inputs are not modified.  stats, if
    a list, receives one dict per (b, c)."""
    conf = np.array(conf, F, copy=True)
    mn, mx = np.asarray(xy_min, F), np.asarray(xy_max, F)
    B, N, C = conf.shape
    check_args(N, method, threshold, threshold_iou, sigma)
    with np.errstate(all='ignore'):
        for b in range(B):
            wh = mx[b] - mn[b]
            area = wh[:, 0] * wh[:, 1]
            for c in range(C):
                st = None if stats is None else {'b': b, 'c': c}
                col = conf[b, :, c].copy()
                conf[b, :, c] = soft_nms_column(col, mn[b], mx[b], area, threshold, threshold_iou, method, sigma, st)
                if stats is not None:
                    stats.append(st)
    return conf, (order_of(conf) if with_order else None)


def order_of(conf):
    """[B,N,C] final scores -> [B,N] box indices by (max over classes descending, index ascending).  The maximum is taken as the kernel
    takes it (v > m ? v : m from class 0 on); -0.0 and +0.0 are equal keys."""
    key = conf[:, :, 0].copy()
    for c in range(1, conf.shape[2]):
        v = conf[:, :, c]
        key = np.where(v > key, v, key)
    return np.stack([np.argsort(-k, kind='stable') for k in key]).astype(np.int64)
