"""Inputs for yolo2_soft_nms (csrc/soft_nms.hip), in the manner of tests/nms_cases.py: a named table of seeded recipes, built once, cached,
read-only.  NumPy only: tests/test_soft_nms_cpu.py checks the table on a machine without a GPU, tests/test_soft_nms_gpu.py launches the
kernel on it.  The expected results are tests/soft_nms_ref.py's (the specification); `paths(name, method)` says which of the kernel's code
paths a case takes, so that the CPU test can assert that the table reaches them all; `model(name, method, mutation)` restates the algorithm
on the full arrays (no compaction) with switches for the ways a kernel could be subtly wrong.

A case is run with every method; `sigma` is the case's Gaussian parameter.  Scores are finite except in `nan_scores`; boxes are finite
with xy_min <= xy_max."""
import functools

import numpy as np

import soft_nms_ref as S
from nms_cases import _boxes, _frozen, bits, pow2_at_least  # noqa: F401  (bits, pow2_at_least: for the tests)

F = np.float32
LDS_DEFAULT = 64 * 1024       # above this yolo2_soft_nms raises hipFuncAttributeMaxDynamicSharedMemorySize
THREADS = 256


def lds_bytes(N):
    """The dynamic LDS request of yolo2_soft_nms (`const size_t lds = ...`): 24 bytes per box (box 16, score 4, index 4), the waves'
    maxima (2 x 4 x 8) and their candidate counts (4 x 4)."""
    return 24 * N + 64 + 16


# 2727 / 2728: the LDS request crosses 64 KiB; 64 / 65: one or two 64-box chunks; 256 / 257: one or two chunks per wave, and (with every
# box a candidate) one or two positions per thread in the pick loop; 513 / 1025: the order kernel's network doubles
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513, 845, 1025, 2727, 2728, 4095, 4096)
COUNTS = (0, 1, 2, 64, 65, 256, 257)
assert lds_bytes(2727) <= LDS_DEFAULT < lds_bytes(2728)

# name -> (B, N, C, threshold, threshold_iou, sigma, recipe, seed, with_order)
CASES = {}
for _i, _n in enumerate(SIZES):
    CASES['n%d' % _n] = (2 if _n < 2000 else 1, _n, 3, 0.3, 0.45, 0.5, 'distinct', 1100 + _i, True)      # (one image at the large sizes: the CPU side's time)
for _i, _k in enumerate(COUNTS):
    CASES['k%d' % _k] = (2, 300, 2, 0.3, 0.45, 0.5, 'planted:%d' % _k, 1200 + _i, True)
CASES.update({
    'all_candidates': (2, 300, 2, 0.0, 0.45, 0.5, 'distinct', 1250, True),              # K = N
    'all_candidates_n257': (1, 257, 1, 0.0, 0.45, 0.5, 'distinct', 1251, True),         # K = N = 257: thread 0 owns two positions
    'chain4096': (1, 4096, 1, 0.0, 0.45, 0.5, 'spread', 1252, True),                    # the longest chain: K = N = 4096, C = B = 1
    # ---- thresholds
    'thr_zero': (2, 200, 3, 0.0, 0.45, 0.5, 'zeros', 1301, True),                       # +0.0 and -0.0 scores: never candidates, bits kept
    'eval_regime': (2, 845, 20, 0.005, 0.45, 0.5, 'eval', 1302, True),                  # eval.py -t 0.005 --threshold_iou 0.45
    'thr_equals_score': (2, 200, 3, 0.25, 0.45, 0.5, 'at_threshold', 1303, True),       # 15 % of the scores equal the threshold
    'land_linear': (2, 150, 2, 0.25, 0.4, 0.5, 'land:linear', 1304, True),              # a linear decay lands on / just below / just above the threshold
    'land_gaussian': (2, 150, 2, None, 0.4, 0.5, 'land:gaussian', 1305, True),          # the same for the Gaussian decay (the threshold comes from the recipe)
    'iou_zero': (2, 200, 3, 0.3, 0.0, 0.5, 'distinct', 1306, True),                     # every overlap, 0 included, is >= the threshold
    'iou_one': (2, 200, 3, 0.3, 1.0, 0.5, 'dups5', 1307, True),                         # only exact duplicates reach it
    'iou_above_one': (2, 200, 3, 0.3, 1.5, 0.5, 'dups5', 1308, True),                   # hard and linear change nothing
    'sigma_min': (2, 200, 3, 0.3, 0.45, 1.0 / 64, 'dups5', 1309, True),                 # soft_exp's argument reaches -64
    'sigma_4': (2, 200, 3, 0.3, 0.45, 4.0, 'distinct', 1310, True),
    # ---- ties
    'tie_index': (2, 120, 3, 0.3, 0.45, 0.5, 'tie_index', 1401, True),                  # three score levels: the box index decides
    'tie_by_decay': (2, 160, 2, 0.1, 0.4, 0.5, 'tie_by_decay', 1402, True),             # ties the decay makes, and duplicates decayed alike
    # ---- geometry
    'dups5': (2, 200, 3, 0.3, 0.45, 0.5, 'dups5', 1501, True),                          # IoU exactly 1: linear weight 0, Gaussian soft_exp(-1/sigma)
    'zero_area': (2, 160, 3, 0.3, 0.45, 0.5, 'zero_area', 1502, True),                  # the 1e-10 floor
    'disjoint': (2, 150, 3, 0.3, 0.45, 0.5, 'disjoint', 1503, True),                    # no overlap: every bit unchanged
    'subnormal': (2, 192, 2, 0.0, 0.45, 0.125, 'subnormal', 1504, True),                # products in the f32 subnormal range
    # ---- interface
    'c1': (2, 300, 1, 0.3, 0.45, 0.5, 'distinct', 1601, True),
    'c80_b3': (3, 845, 80, 0.3, 0.45, 0.5, 'sparse', 1602, True),
    'no_order': (2, 300, 3, 0.3, 0.45, 0.5, 'distinct', 1603, False),                   # order_out = NULL
    'side_stream': (2, 300, 3, 0.3, 0.45, 0.5, 'distinct', 1604, True),                 # launched on a non-default stream by the GPU test
    'nan_scores': (2, 200, 3, 0.3, 0.45, 0.5, 'nan', 1605, False),                      # NaN is no candidate and keeps its bits
})
SIDE_STREAM_CASE = 'side_stream'
NAMES = tuple(CASES)
# where every mutation of model() is tried (the unswitched model runs everywhere)
SMALL = tuple(n for n in NAMES if CASES[n][1] * CASES[n][2] <= 1000)


# ---------------------------------------------------------------------------------------------------------------------
# recipes: (rng, B, N, C, thr) -> conf, xy_min, xy_max[, threshold]
# ---------------------------------------------------------------------------------------------------------------------

def _distinct_scores(rng, B, N, C, lo=0.01, hi=0.99):
    """Every class column a permutation of N evenly spaced values: no two scores of a class tie."""
    levels = np.linspace(lo, hi, N).astype(F)
    assert N == 1 or len(np.unique(levels)) == N
    conf = np.empty((B, N, C), F)
    for b in range(B):
        for c in range(C):
            conf[b, :, c] = levels[rng.permutation(N)]
    return conf


def _recipe_distinct(rng, B, N, C, thr):
    return (_distinct_scores(rng, B, N, C),) + _boxes(rng, B, N)


def _recipe_spread(rng, B, N, C, thr):
    return (_distinct_scores(rng, B, N, C),) + _boxes(rng, B, N, 40.0)


def _recipe_planted(rng, B, N, C, thr, K):
    """Exactly K scores of class 0 above the threshold, all distinct; the others at or below it (a twentieth exactly at it)."""
    conf = _distinct_scores(rng, B, N, C)
    mn, mx = _boxes(rng, B, N, 6.0)
    for b in range(B):
        col = rng.uniform(0, thr - 0.01, N).astype(F)
        col[rng.rand(N) < 0.05] = F(thr)
        hot = rng.choice(N, K, replace=False)
        col[hot] = np.linspace(thr + 0.01, 0.97, max(K, 1)).astype(F)[rng.permutation(K)] if K else col[hot]
        conf[b, :, 0] = col
    return conf, mn, mx


def _recipe_zeros(rng, B, N, C, thr):
    conf = _distinct_scores(rng, B, N, C)
    z = rng.rand(B, N, C)
    conf[z < 0.15] = F(0.0)
    conf[(z >= 0.15) & (z < 0.30)] = F(-0.0)
    return (conf,) + _boxes(rng, B, N)


def _recipe_at_threshold(rng, B, N, C, thr):
    conf = _distinct_scores(rng, B, N, C)
    conf[rng.rand(B, N, C) < 0.15] = F(thr)
    return (conf,) + _boxes(rng, B, N)


def _recipe_eval(rng, B, N, C, thr):
    """tests/nms_cases.py's eval recipe: scores skewed as a detector's are (0.9 u^8), 2 % at the threshold, 40 confident ones per image."""
    conf = (rng.uniform(0, 1, (B, N, C)) ** 8 * 0.9).astype(F)
    conf[rng.rand(B, N, C) < 0.02] = F(0.005)
    for b in range(B):
        hot = rng.choice(N, 40, replace=False)
        conf[b, hot, rng.randint(0, C, 40)] = rng.uniform(0.3, 0.95, 40).astype(F)
    return (conf,) + _boxes(rng, B, N)


def _recipe_sparse(rng, B, N, C, thr):
    conf = rng.uniform(0, 0.05, (B, N, C)).astype(F)
    for b in range(B):
        hot = rng.choice(N, 40, replace=False)
        conf[b, hot, rng.randint(0, C, 40)] = rng.uniform(0.3, 0.95, 40).astype(F)
    return (conf,) + _boxes(rng, B, N)


def _recipe_dups5(rng, B, N, C, thr):
    assert N % 5 == 0
    mn, mx = _boxes(rng, B, N // 5, 13.0)
    pick = np.stack([rng.permutation(np.repeat(np.arange(N // 5), 5)) for _ in range(B)])
    mn = np.stack([mn[b, pick[b]] for b in range(B)])
    mx = np.stack([mx[b, pick[b]] for b in range(B)])
    return _distinct_scores(rng, B, N, C), mn, mx


def _recipe_tie_index(rng, B, N, C, thr):
    conf = rng.choice(F([0.1, 0.35, 0.6]), (B, N, C)).astype(F)
    return (conf,) + _boxes(rng, B, N, 6.0)


def _recipe_zero_area(rng, B, N, C, thr):
    """A quarter each: zero width, zero height, zero area at one of four shared points (identical boxes), ordinary."""
    mn, mx = _boxes(rng, B, N, 5.0)
    kind = np.arange(N) % 4
    mx[:, kind == 0, 0] = mn[:, kind == 0, 0]
    mx[:, kind == 1, 1] = mn[:, kind == 1, 1]
    points = rng.uniform(1, 4, (B, 4, 2)).astype(F)
    at = points[:, rng.randint(0, 4, (kind == 2).sum())]
    mn[:, kind == 2] = at
    mx[:, kind == 2] = at
    return _distinct_scores(rng, B, N, C), mn, mx


def _recipe_disjoint(rng, B, N, C, thr):
    cell = np.stack([3 * (np.arange(N) % 16), 3 * (np.arange(N) // 16)], 1).astype(F)
    mn = np.stack([cell[rng.permutation(N)] for _ in range(B)])
    return _distinct_scores(rng, B, N, C), mn, mn + F(2)


def _recipe_nan(rng, B, N, C, thr):
    conf = _distinct_scores(rng, B, N, C)
    conf[rng.rand(B, N, C) < 0.1] = F(np.nan)
    return (conf,) + _boxes(rng, B, N)


def _motifs(rng, B, N, per, place):
    """N / per copies of a `per`-box motif, 10 apart, the boxes of each image in a random order.  place(b, m, slots) fills copy m, whose boxes
    have the indices `slots`."""
    assert N % per == 0
    M = N // per
    off = np.stack([10.0 * (np.arange(M) % 8), 10.0 * (np.arange(M) // 8)], 1).astype(F)
    for b in range(B):
        where = rng.permutation(N).reshape(M, per)
        for m in range(M):
            place(b, m, where[m], off[m])


def _recipe_tie_by_decay(rng, B, N, C, thr):
    """Motif of four: A = [0,0]-[2,1] with 0.9; Z1 = Z2 = [0,0]-[1,1] (IoU with A exactly 1/2) with equal scores 0.8; Y far from them with
    0.4.  Linear at threshold_iou 0.4: A's pick halves Z1 and Z2 to 0.4, a tie with Y that did not exist before, and with each other; the box
    index decides among the three.  Gaussian: Z1 and Z2 decay by the same factor and stay tied.  Class 1 has the roles' scores scaled."""
    conf = np.zeros((B, N, C), F)
    mn, mx = np.zeros((B, N, 2), F), np.zeros((B, N, 2), F)

    def place(b, m, slots, off):
        a, z1, z2, y = slots
        mn[b, a], mx[b, a] = off, off + F([2, 1])
        mn[b, z1], mx[b, z1] = off, off + F([1, 1])
        mn[b, z2], mx[b, z2] = off, off + F([1, 1])
        mn[b, y], mx[b, y] = off + F([5, 5]), off + F([6, 6])
        conf[b, [a, z1, z2, y], 0] = F([0.9, 0.8, 0.8, 0.4])
        conf[b, [a, z1, z2, y], 1] = F([0.45, 0.4, 0.4, 0.2]) if m % 2 else F([0.9, 0.5, 0.5, 0.25])
    _motifs(rng, B, N, 4, place)
    return conf, mn, mx


def _recipe_land(rng, B, N, C, thr, method):
    """Motif of three: A = [0,0]-[2,1] with 0.9, T0 = [0,0]-[1,1] and T1 = [1,0]-[2,1]: each has IoU exactly 1/2 with A and none with the
    other.  With w the weight of IoU 1/2, the scores of T0 / T1 are two of (`on`, just below it, just above it), rotating with the copy, so
    that A's pick moves them exactly onto the threshold t = on * w (not kept: `>`), just below it and just above it.  linear: w = 1/2,
    t = 0.25; gaussian: t is returned, computed with soft_exp; on = 0.5, so the product is exact."""
    on = F(0.5)
    w = F(0.5) if method == 'linear' else S.soft_exp(-((F([0.5]) * F(0.5)) / F(0.5)))[0]
    t = on * w
    below, above = np.nextafter(on, F(0)), np.nextafter(on, F(1))
    # (round-to-even can put a neighbour's product on t itself: move on until the three results are below, at and above)
    while not below * w < t:
        below = np.nextafter(below, F(0))
    while not above * w > t:
        above = np.nextafter(above, F(1))
    trio = F([on, below, above])
    conf = np.zeros((B, N, C), F)
    mn, mx = np.zeros((B, N, 2), F), np.zeros((B, N, 2), F)

    def place(b, m, slots, off):
        a, t0, t1 = slots
        mn[b, a], mx[b, a] = off, off + F([2, 1])
        mn[b, t0], mx[b, t0] = off, off + F([1, 1])
        mn[b, t1], mx[b, t1] = off + F([1, 0]), off + F([2, 1])
        conf[b, a, :] = F(0.9)
        conf[b, t0, :], conf[b, t1, :] = trio[m % 3], trio[(m + 1) % 3]
    _motifs(rng, B, N, 3, place)
    return conf, mn, mx, float(t)


def _recipe_subnormal(rng, B, N, C, thr):
    """Sixteen-fold duplicates.  Class 0: scores near 1, sigma 1/8: a duplicate's Gaussian weight is soft_exp(-8) = 3.4e-4 and the j-th of a
    group has been decayed j - 1 times: the 12th and 13th are subnormal, the 14th underflows.  Class 1: scores of 1.25e-38 .. 2.5e-38 (normal,
    above threshold 0) and boxes that also overlap partly, so linear weights 1 - IoU take them below 1.18e-38."""
    assert N % 16 == 0
    G = N // 16
    cen = rng.uniform(0, 6, (B, G, 2)).astype(F)
    wh = rng.uniform(2, 4, (B, G, 2)).astype(F)
    gmn, gmx = (cen - wh / 2).astype(F), (cen + wh / 2).astype(F)
    pick = np.stack([rng.permutation(np.repeat(np.arange(G), 16)) for _ in range(B)])
    mn = np.stack([gmn[b, pick[b]] for b in range(B)])
    mx = np.stack([gmx[b, pick[b]] for b in range(B)])
    conf = _distinct_scores(rng, B, N, C, 0.5, 0.99)
    conf[:, :, 1] = (conf[:, :, 1] * F(2.5e-38)).astype(F)
    assert conf[:, :, 1].min() >= np.finfo(F).tiny and len(np.unique(conf[0, :, 1])) == N
    return conf, mn, mx


RECIPES = {'distinct': _recipe_distinct, 'spread': _recipe_spread, 'zeros': _recipe_zeros, 'at_threshold': _recipe_at_threshold, 'eval': _recipe_eval,
           'sparse': _recipe_sparse, 'dups5': _recipe_dups5, 'tie_index': _recipe_tie_index, 'zero_area': _recipe_zero_area,
           'disjoint': _recipe_disjoint, 'nan': _recipe_nan, 'tie_by_decay': _recipe_tie_by_decay, 'subnormal': _recipe_subnormal}


@functools.lru_cache(maxsize=None)
def case(name):
    """{'name', 'B', 'N', 'C', 'thr', 'thr_iou', 'sigma', 'with_order', 'conf' [B,N,C], 'xy_min', 'xy_max' [B,N,2]}: f32, read-only."""
    B, N, C, thr, thr_iou, sigma, recipe, seed, with_order = CASES[name]
    rng = np.random.RandomState(seed)
    kind, _, arg = recipe.partition(':')
    if kind == 'planted':
        out = _recipe_planted(rng, B, N, C, thr, int(arg))
    elif kind == 'land':
        out = _recipe_land(rng, B, N, C, thr, arg)
    else:
        out = RECIPES[kind](rng, B, N, C, thr)
    if len(out) == 4:
        assert thr is None or float(F(thr)) == out[3]
        thr = out[3]
    conf, mn, mx = out[:3]
    assert conf.shape == (B, N, C) and mn.shape == mx.shape == (B, N, 2)
    assert conf.dtype == mn.dtype == mx.dtype == F
    assert kind == 'nan' or np.all(np.isfinite(conf))
    assert np.all(np.isfinite(mn)) and np.all(np.isfinite(mx)) and np.all(mn <= mx)
    # the kernel takes the thresholds as floats: what it compares with is the f32 value
    return {'name': name, 'B': B, 'N': N, 'C': C, 'thr': float(F(thr)), 'thr_iou': float(F(thr_iou)), 'sigma': float(F(sigma)),
            'with_order': with_order, 'conf': _frozen(conf), 'xy_min': _frozen(mn), 'xy_max': _frozen(mx)}


@functools.lru_cache(maxsize=None)
def _reference(name, method):
    c = case(name)
    stats = []
    conf, order = S.soft_nms(c['conf'], c['xy_min'], c['xy_max'], c['thr'], c['thr_iou'], method, c['sigma'], c['with_order'], stats)
    for st in stats:
        K = st['K']
        st.update(N=c['N'], per=-(-K // THREADS), chunks=-(-c['N'] // 64), chunks_per_wave=-(-(-(-c['N'] // 64)) // 4), lds_bytes=lds_bytes(c['N']),
                  lds_raised=lds_bytes(c['N']) > LDS_DEFAULT, NP=pow2_at_least(c['N'], 2))
    return _frozen(conf), (None if order is None else _frozen(order)), tuple(stats)


def reference(name, method):
    """The specification on a case: (conf_out [B,N,C] f32, order [B,N] int64 or None), read-only."""
    return _reference(name, method)[:2]


def paths(name, method):
    """What the kernel goes through on this case, one dict per (image b, class c): K (candidates), picks, zeroed (candidates written as +0),
    per (positions per thread in the pick loop), chunks / chunks_per_wave (the compaction's 64-box chunks), NP (the order network),
    lds_bytes / lds_raised, decay_ties (picks before which a tie at the top existed that the decay made), subnormal (a product fell into
    the subnormal range), floor (a union at the 1e-10 floor)."""
    return _reference(name, method)[2]


def tie_free(name):
    """No two candidates of any (image, class) have equal scores: hard Soft-NMS and the reference's NMS then pick in the same order."""
    c = case(name)
    conf = c['conf']
    for b in range(c['B']):
        for k in range(c['C']):
            col = conf[b, :, k]
            cand = col[col > F(c['thr'])]
            if len(np.unique(cand)) != len(cand):
                return False
    return True


# ---------------------------------------------------------------------------------------------------------------------
# the algorithm restated on the full arrays, with switches
# ---------------------------------------------------------------------------------------------------------------------

MUTATIONS = ('single_sort', 'ties_high_index', 'decay_picked', 'decay_noncand', 'gt_iou', 'stop_early', 'write_decayed')


def _weight(iou, method, thr_iou, sigma, mutation):
    if mutation == 'gt_iou' and method != 'gaussian':
        hit = iou > thr_iou
        return np.where(hit, F(0) if method == 'hard' else F(1) - iou, F(1)).astype(F)
    return S.weight(iou, method, thr_iou, sigma)


def _model_column(s0, mn, mx, area, thr, thr_iou, method, sigma, mutation):
    N = len(s0)
    s = s0.copy()
    cand = s > thr
    picked = np.zeros(N, bool)
    everything = np.arange(N)
    sequence = []
    if mutation == 'single_sort':
        # the classic formulation: one sort by the ORIGINAL scores, then a walk that never looks back at the order
        walk = [i for i in everything[np.lexsort((everything, -s0))] if cand[i]]
    while True:
        open_ = cand & ~picked
        if mutation == 'single_sort':
            walk = [i for i in walk if not picked[i]]
            while walk and not (s[walk[0]] > thr):
                walk.pop(0)                                  # decayed away: the walk passes it
            if not walk:
                break
            m = walk[0]
        else:
            if not open_.any():
                break
            idx = everything[open_]
            top = idx[s[idx] == s[idx].max()]
            m = top[-1] if mutation == 'ties_high_index' else top[0]
            if not (s[m] > thr):
                break
        picked[m] = True
        sequence.append(m)
        targets = everything[~picked] if mutation == 'decay_noncand' else everything[cand & ~picked]
        if mutation == 'decay_picked':
            targets = np.sort(np.append(targets, m))
        if len(targets):
            s[targets] = s[targets] * _weight(S.iou_with(mn, mx, area, m, targets), method, thr_iou, sigma, mutation)
    if mutation == 'stop_early' and sequence:
        picked[sequence[-1]] = False
    out = s0.copy()
    out[cand] = F(0)
    out[picked] = s[picked]
    if mutation == 'write_decayed':
        out[cand & ~picked] = s[cand & ~picked]
    if mutation == 'decay_noncand':
        out[~cand] = s[~cand]
    return out


@functools.lru_cache(maxsize=None)
def model(name, method, mutation=None):
    """The restated algorithm on a case: (conf_out [B,N,C], order [B,N] or None).  `mutation` is None or one of MUTATIONS."""
    assert mutation is None or mutation in MUTATIONS
    c = case(name)
    conf = c['conf'].copy()
    thr, thr_iou, sigma = F(c['thr']), F(c['thr_iou']), F(c['sigma'])
    with np.errstate(all='ignore'):
        for b in range(c['B']):
            mn, mx = c['xy_min'][b], c['xy_max'][b]
            wh = mx - mn
            area = wh[:, 0] * wh[:, 1]
            for k in range(c['C']):
                conf[b, :, k] = _model_column(c['conf'][b, :, k], mn, mx, area, thr, thr_iou, method, sigma, mutation)
    return _frozen(conf), (_frozen(S.order_of(conf)) if c['with_order'] else None)
